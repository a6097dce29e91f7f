"""Host-side mirror of the reference's interface for the Path hot path.

Names, argument meaning and error behaviour follow yuki's Rust types so that the
parity tests read like the reference's call sites:

    FilmSettings / FilmTile / film_tiles      yuki/src/film.rs:14-65,409-475
    CameraParameters / FoV / Camera           yuki/src/camera.rs:19-114
    SamplerType.Uniform / .Stratified         yuki/src/sampling/mod.rs:16-31
    IntegratorType.Path(PathParams) ...       yuki/src/integrators/mod.rs:33-53
    Integrator.render(scene, camera, sampler, tile) -> (tile_pixels, ray_count)
                                              yuki/src/integrators/mod.rs:120-185
    Scene                                     yuki/src/scene/mod.rs:41-49

Everything computes through libyuki_hip.so (the C ABI of include/yuki_hip.h);
this file only marshals arguments.  The reference panics on contract
violations; here they surface as YukiError carrying the yk_status.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _ffi, abi
from ._ffi import BvhBuildInfo, RenderStats, SceneInfo, YukiError, check, lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _vp(a):
    """A device address or a stream handle as a c_void_p; None or 0 — an array the call leaves out, the context's own
    stream — as None (NULL)."""
    return C.c_void_p(a) if a else None


def _film(film):
    """An (h, w, 3) float32 film -> (film, w, h), the film C-contiguous."""
    film = np.ascontiguousarray(film, dtype=np.float32)
    if film.ndim != 3 or film.shape[2] != 3:
        raise ValueError("film is (h, w, 3)")
    return film, film.shape[1], film.shape[0]


def _scene_diagonal(scene):
    """The diagonal of the scene's bounds (Scene.info()): what the for_scene constructors scale their plane stops by."""
    i = scene.info()
    return float(np.linalg.norm(np.array(i.bounds_max[:], dtype=np.float64) - np.array(i.bounds_min[:], dtype=np.float64)))


# --------------------------------------------------------------------------- film
@dataclass
class FilmSettings:
    """film.rs:14-39 (defaults :28-38)."""

    res: tuple = (640, 480)
    tile_dim: int = 16
    clear: bool = True
    accumulate: bool = False
    sixteenth_res: bool = False


@dataclass
class FilmTile:
    """film.rs:43-65 — `bb` is (x0, y0, x1, y1), max exclusive."""

    bb: tuple
    sample: int = 0

    def as_struct(self):
        return abi.Tile(*[int(v) for v in self.bb])


def film_tiles(settings: FilmSettings):
    """film.rs:409-475: clipped tiles in outward-spiral order (numpy TILE_DTYPE)."""
    L = lib()
    n = L.yk_film_tiles(settings.res[0], settings.res[1], settings.tile_dim, None, 0)
    t = np.zeros(n, dtype=abi.TILE_DTYPE)
    L.yk_film_tiles(settings.res[0], settings.res[1], settings.tile_dim, _p(t), n)
    return t


def multi_deal(settings: FilmSettings, n_ranks, rank):
    """yk_multi_deal: the tiles of `rank` among `n_ranks` (spiral tile i -> rank i mod n_ranks, render_manager.rs:206-210)
    and the rank's pixel count; needs no device."""
    L = lib()
    px = C.c_uint64(0)
    n = L.yk_multi_deal(settings.res[0], settings.res[1], settings.tile_dim, n_ranks, rank, None, 0, C.byref(px))
    t = np.zeros(n, dtype=abi.TILE_DTYPE)
    L.yk_multi_deal(settings.res[0], settings.res[1], settings.tile_dim, n_ranks, rank, _p(t), n, C.byref(px))
    return t, int(px.value)


def update_tiles(tiles, tile_rgb, res):
    """Film::update_tile (film.rs:210-282) for a list of tiles: tile-major -> row-major."""
    tiles = np.ascontiguousarray(tiles, dtype=abi.TILE_DTYPE)
    tile_rgb = np.ascontiguousarray(tile_rgb, dtype=np.float32)
    film = np.zeros((res[1], res[0], 3), dtype=np.float32)
    check(lib().yk_film_update_tiles(_p(tiles), len(tiles), _p(tile_rgb), res[0], res[1], _p(film)))
    return film


def accumulate_tiles(tiles, tile_rgb, film, tile_sample_counts=None):
    """Film::update_tile with accumulation on (film.rs:260-272): film += tile pixels, in place;
    tile_sample_counts[t] += 1."""
    tiles = np.ascontiguousarray(tiles, dtype=abi.TILE_DTYPE)
    tile_rgb = np.ascontiguousarray(tile_rgb, dtype=np.float32)
    assert film.dtype == np.float32 and film.flags["C_CONTIGUOUS"]
    if tile_sample_counts is not None:
        assert tile_sample_counts.dtype == np.uint32 and len(tile_sample_counts) == len(tiles)
    check(lib().yk_film_accumulate_tiles(_p(tiles), len(tiles), _p(tile_rgb), film.shape[1], film.shape[0], _p(film), _p(tile_sample_counts)))
    return film


def write_exr(path, film):
    """app/util.rs:90-111 write_exr: (h, w, 3) float32 -> RGB OpenEXR file."""
    film = np.ascontiguousarray(film, dtype=np.float32)
    check(lib().yk_write_exr(str(path).encode(), film.shape[1], film.shape[0], _p(film)))


def write_pfm(path, film):
    film = np.ascontiguousarray(film, dtype=np.float32)
    check(lib().yk_write_pfm(str(path).encode(), film.shape[1], film.shape[0], _p(film)))


# --------------------------------------------------------------------------- tone map
@dataclass
class FilmicParams:
    """app/renderpasses/tonemap.rs:12-22."""

    exposure: float = 1.0


class HeatmapChannel:
    """tonemap.rs:53-59."""

    Red, Green, Blue, Luminance = abi.HEATMAP_RED, abi.HEATMAP_GREEN, abi.HEATMAP_BLUE, abi.HEATMAP_LUMINANCE


@dataclass
class HeatmapParams:
    """tonemap.rs:24-38: bounds None = find_min_max over the film first (app/headless.rs:135-145)."""

    bounds: tuple = None
    channel: int = HeatmapChannel.Red


class ToneMapType:
    """tonemap.rs:40-51; the semantics are stated in yuki_amd/csrc/yk_tonemap.h."""

    Raw = abi.ToneMapDesc(abi.TONE_MAP_RAW, 1.0, 0, 0, (C.c_float * 2)(0.0, 0.0))

    @staticmethod
    def Filmic(params: FilmicParams = None):
        params = params or FilmicParams()
        return abi.ToneMapDesc(abi.TONE_MAP_FILMIC, params.exposure, 0, 0, (C.c_float * 2)(0.0, 0.0))

    @staticmethod
    def Heatmap(params: HeatmapParams = None):
        params = params or HeatmapParams()
        b = (0.0, 0.0) if params.bounds is None else params.bounds
        return abi.ToneMapDesc(abi.TONE_MAP_HEATMAP, 1.0, int(params.channel), 0 if params.bounds is None else 1, (C.c_float * 2)(*[float(v) for v in b]))

    @staticmethod
    def default():
        return ToneMapType.Filmic(FilmicParams())


def film_tile_dim(settings: FilmSettings):
    """Film::tile_dim() (film.rs:143-150) as the tone map reads it (tonemap.rs:238): the width of the first tile of the
    spiral queue (film.rs:173-181), 16 without tiles.  It differs from settings.tile_dim only for a film narrower than a tile."""
    t = film_tiles(settings)
    return 16 if len(t) == 0 else int(t[0]["x1"]) - int(t[0]["x0"])


def _table_len(res, tile_dim):
    return (-(-int(res[0]) // tile_dim)) * (-(-int(res[1]) // tile_dim))


def film_samples(settings: FilmSettings, tiles, counts):
    """Film.samples (film.rs:74, 260-272) from per-tile counts.  accumulate_tiles counts by POSITION in `tiles` (spiral
    order); the table is in FilmTile.index order (generate_tiles, film.rs:299-331): (y0 / td) * ceil(W / td) + x0 / td."""
    tiles = np.ascontiguousarray(tiles, dtype=abi.TILE_DTYPE)
    counts = np.asarray(counts, dtype=np.uint32)
    if len(counts) != len(tiles):
        raise ValueError("one count per tile")
    td = int(settings.tile_dim)
    cols = -(-int(settings.res[0]) // td)
    table = np.zeros(_table_len(settings.res, td), dtype=np.uint32)
    idx = (tiles["y0"].astype(np.int64) // td) * cols + tiles["x0"].astype(np.int64) // td
    np.add.at(table, idx, counts)
    return table


def _tone_map_args(res, tone_map, tile_dim, samples):
    if not isinstance(tone_map, abi.ToneMapDesc):
        raise TypeError("tone_map is a ToneMapType")
    if samples is not None:
        samples = np.ascontiguousarray(samples, dtype=np.uint32)
        if int(tile_dim) > 0 and samples.size != _table_len(res, int(tile_dim)):
            raise ValueError(f"samples has {samples.size} entries, the film's tile grid {_table_len(res, int(tile_dim))}")
    return samples


def _metered(desc, exposure_state):
    """The Filmic descriptor whose exposure is desc.exposure * exposure_state.exposure, the one binary32 multiply of
    yk_tone_map_metered_device."""
    if desc.kind != abi.TONE_MAP_FILMIC:
        raise ValueError("exposure_state needs the Filmic tone map: the others have no exposure")
    e = np.float32(desc.exposure) * np.float32(exposure_state.exposure)
    return abi.ToneMapDesc(abi.TONE_MAP_FILMIC, float(e), 0, 0, (C.c_float * 2)(0.0, 0.0))


def tone_map(film, tone_map, tile_dim, samples=None, ctx=None, used_bounds=None, exposure_state=None):
    """ToneMapFilm::draw (tonemap.rs:143-213) plus the bounds search of headless.rs:135-145: (h, w, 3) float32 in and out.
    ctx None = the host instance; `used_bounds` (a float32[2] array) receives the Heatmap bounds applied.  exposure_state
    (an ExposureState, Filmic only): the exposure is the descriptor's times the meter's."""
    if exposure_state is not None:
        tone_map = _metered(tone_map, exposure_state)
    return _apply_tone_map(film, tone_map, tile_dim, samples, ctx, used_bounds)


def _apply_tone_map(film, desc, tile_dim, samples, ctx, used_bounds):
    film = np.ascontiguousarray(film, dtype=np.float32)
    h, w = film.shape[0], film.shape[1]
    samples = _tone_map_args((w, h), desc, tile_dim, samples)
    out = np.empty_like(film)
    c = ctx.h if ctx else None
    check(lib().yk_tone_map(c, C.byref(desc), _p(film), w, h, int(tile_dim), _p(samples), _p(out), _p(used_bounds)), c)
    return out


def find_min_max(film, channel, ctx=None):
    """tonemap.rs:447-472: (min, max) of a channel (or luminance) over the film, NaN pixels skipped."""
    film = np.ascontiguousarray(film, dtype=np.float32)
    out = np.zeros(2, dtype=np.float32)
    c = ctx.h if ctx else None
    check(lib().yk_film_min_max(c, _p(film), film.shape[1], film.shape[0], int(channel), _p(out)), c)
    return float(out[0]), float(out[1])


# --------------------------------------------------------------------------- exposure meter
@dataclass
class ExposureParams:
    """yk_exposure_desc (csrc/yk_exposure.h): low_cut / high_cut are the fractions of the counted pixels dropped at the
    dark and the bright end (converted by round(x * 65536)); the metered luminance is brought to `key`, `compensation`
    stops brighter; the stops applied stay in [min_ev, max_ev]; adapt_up / adapt_down are the per-frame rates (1 = at
    once) towards a brighter / a darker film; window (x0, y0, x1, y1), half open, None = the whole film."""

    low_cut: float = 0.05
    high_cut: float = 0.02
    key: float = 0.18
    compensation: float = 0.0
    min_ev: float = -8.0
    max_ev: float = 8.0
    adapt_up: float = 1.0
    adapt_down: float = 1.0
    window: tuple = None

    def desc(self, res):
        w = (0, 0, int(res[0]), int(res[1])) if self.window is None else tuple(int(v) for v in self.window)
        if len(w) != 4 or min(w) < 0 or max(w) > 65535:
            raise ValueError("window is (x0, y0, x1, y1) in pixels")
        ev_bias = float(np.log2(self.key)) + float(self.compensation)
        return abi.ExposureDesc(int(round(self.low_cut * 65536)), int(round(self.high_cut * 65536)), ev_bias, self.min_ev, self.max_ev, self.adapt_up, self.adapt_down, (C.c_uint16 * 4)(*w))


ExposureState = abi.ExposureState


def _window(window):
    if window is None:
        return None
    w = tuple(int(v) for v in window)
    if len(w) != 4 or min(w) < 0 or max(w) > 65535:
        raise ValueError("window is (x0, y0, x1, y1) in pixels")
    return (C.c_uint16 * 4)(*w)


def film_histogram(film, tile_dim, samples=None, window=None, ctx=None):
    """yk_film_histogram: the meter's 256 luminance bins of an (h, w, 3) float32 film (uint32) and the (skipped, below,
    above) counts, by the rule of csrc/yk_exposure.h.  ctx None = the host instance."""
    film, w, h = _film(film)
    samples = _tone_map_args((w, h), ToneMapType.Raw, tile_dim, samples)
    bins = np.zeros(256, dtype=np.uint32)
    sba = np.zeros(3, dtype=np.uint32)
    c = ctx.h if ctx else None
    check(lib().yk_film_histogram(c, _p(film), w, h, int(tile_dim), _p(samples), _window(window), _p(bins), _p(sba)), c)
    return bins, tuple(int(v) for v in sba)


def meter_exposure(film, tile_dim, params=None, samples=None, prev=None, ctx=None):
    """yk_exposure_meter: the ExposureState of an (h, w, 3) float32 film under `params` (None = ExposureParams()), after
    `prev` (an ExposureState, None = no history).  ctx None = the host instance."""
    film, w, h = _film(film)
    samples = _tone_map_args((w, h), ToneMapType.Raw, tile_dim, samples)
    d = (params or ExposureParams()).desc((w, h))
    out = ExposureState()
    c = ctx.h if ctx else None
    check(lib().yk_exposure_meter(c, C.byref(d), _p(film), w, h, int(tile_dim), _p(samples), None if prev is None else C.byref(prev), C.byref(out)), c)
    return out


def _auto_exposure(film, tone_map, auto_exposure, tile_dim, samples, ctx):
    """The metered descriptor of write_output / write_preview: auto_exposure is True or an ExposureParams."""
    if not auto_exposure:
        return tone_map
    params = ExposureParams() if auto_exposure is True else auto_exposure
    return _metered(tone_map, meter_exposure(film, tile_dim, params, samples, None, ctx))


# --------------------------------------------------------------------------- denoise
@dataclass
class DenoiseParams:
    """yk_denoise_desc: the à-trous iterations (0 .. 8) and the colour, normal and plane-distance stops of
    csrc/yk_denoise.h; float("inf") switches a stop off.  sigma_plane is in scene units: None stands for "no plane stop"
    (+inf); DenoiseParams.for_scene scales it to the scene."""

    iterations: int = 5
    sigma_color: float = 4.0
    sigma_normal: float = 0.3
    sigma_plane: float = None

    @staticmethod
    def for_scene(scene, **kw):
        """sigma_plane = 0.01 x the diagonal of the scene's bounds (Scene.info())."""
        return DenoiseParams(sigma_plane=0.01 * _scene_diagonal(scene), **kw)

    def as_struct(self):
        return abi.DenoiseDesc(int(self.iterations), float(self.sigma_color), float(self.sigma_normal), float("inf") if self.sigma_plane is None else float(self.sigma_plane))


def _denoise_args(res, params, guides, tile_dim, samples):
    if not isinstance(params, DenoiseParams):
        raise TypeError("params is a DenoiseParams")
    samples = _blend_samples(res, tile_dim, samples)
    if guides is not None:
        guides = np.ascontiguousarray(guides, dtype=abi.GUIDE_DTYPE)
        if guides.size != int(res[0]) * int(res[1]):
            raise ValueError("one guide record per film pixel")
    return params.as_struct(), guides, samples


def render_guides(ctx, scene, camera, film_settings):
    """yk_render_guides: the first-hit geometry of the ray through every pixel centre as an (h, w) array of
    abi.GUIDE_DTYPE records (ns, hit, p, t); a miss is an all-zero record."""
    w, h = film_settings.res
    out = np.zeros((h, w), dtype=abi.GUIDE_DTYPE)
    check(lib().yk_render_guides(ctx.h, scene.h, C.byref(camera.matrices), w, h, _p(out)), ctx.h)
    return out


def denoise(film, guides, params, tile_dim=16, samples=None, ctx=None, albedo=None, variance=None):
    """yk_denoise: the edge-avoiding à-trous filter of csrc/yk_denoise.h over an (h, w, 3) float32 film under (h, w)
    guides; `samples` = Film.samples (film_samples) for an accumulating film, whose sums are normalised first.  Returns the
    new film; ctx None = the host instance.  albedo (surface_albedo's (h, w) records): yk_denoise_albedo, the same filter
    on radiance / albedo (csrc/yk_albedo.h).  variance (variance()'s (h, w) image) with a VarianceParams:
    yk_denoise_variance, whose colour stop follows the variance (csrc/yk_variance.h); albedo is honoured there too."""
    film, w, h = _film(film)
    if variance is not None or isinstance(params, VarianceParams):
        if variance is None:
            raise ValueError("a VarianceParams needs variance (variance())")
        d = _variance_desc(params)
        samples = _blend_samples((w, h), tile_dim, samples)
        guides = _records(guides, abi.GUIDE_DTYPE, (w, h), "guide")
        variance = np.ascontiguousarray(variance, dtype=np.float32)
        if variance.size != w * h:
            raise ValueError("one variance per film pixel")
        if albedo is not None:
            albedo = _records(albedo, abi.ALBEDO_DTYPE, (w, h), "albedo")
        out = np.empty_like(film)
        c = ctx.h if ctx else None
        check(lib().yk_denoise_variance(c, C.byref(d), _p(film), _p(guides), _p(variance), _p(albedo), w, h, int(tile_dim), _p(samples), _p(out)), c)
        return out
    d, guides, samples = _denoise_args((w, h), params, guides, tile_dim, samples)
    out = np.empty_like(film)
    c = ctx.h if ctx else None
    if albedo is not None:
        albedo = _records(albedo, abi.ALBEDO_DTYPE, (w, h), "albedo")
        check(lib().yk_denoise_albedo(c, C.byref(d), _p(film), _p(guides), _p(albedo), w, h, int(tile_dim), _p(samples), _p(out)), c)
        return out
    check(lib().yk_denoise(c, C.byref(d), _p(film), _p(guides), w, h, int(tile_dim), _p(samples), _p(out)), c)
    return out


# --------------------------------------------------------------------------- temporal
@dataclass
class TemporalParams:
    """yk_temporal_desc: the plane and normal tests of reproject_history and the history clamp of blend_history
    (csrc/yk_temporal.h).  plane_tolerance is in scene units: None stands for "no plane test" (+inf);
    TemporalParams.for_scene scales it to the scene."""

    plane_tolerance: float = None
    normal_cos_min: float = 0.9
    max_history: float = 64.0

    @staticmethod
    def for_scene(scene, **kw):
        """plane_tolerance = 0.01 x the diagonal of the scene's bounds (Scene.info()), as DenoiseParams.for_scene."""
        return TemporalParams(plane_tolerance=0.01 * _scene_diagonal(scene), **kw)

    def as_struct(self):
        return abi.TemporalDesc(float("inf") if self.plane_tolerance is None else float(self.plane_tolerance), float(self.normal_cos_min), float(self.max_history))


def _temporal_desc(params):
    if not isinstance(params, TemporalParams):
        raise TypeError("params is a TemporalParams")
    return params.as_struct()


def _records(a, dtype, res, what):
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.size != int(res[0]) * int(res[1]):
        raise ValueError(f"one {what} record per film pixel")
    return a


def reproject_history(history, prev_guides, prev_camera, guides, params, ctx=None):
    """yk_history_reproject: the (h, w) abi.HISTORY_DTYPE history of the previous view, its guides and its Camera, and the
    current view's guides -> the history as the current view sees it.  ctx None = the host instance."""
    guides = np.ascontiguousarray(guides, dtype=abi.GUIDE_DTYPE)
    if guides.ndim != 2:
        raise ValueError("guides is (h, w)")
    h, w = guides.shape
    history = _records(history, abi.HISTORY_DTYPE, (w, h), "history")
    prev_guides = _records(prev_guides, abi.GUIDE_DTYPE, (w, h), "guide")
    d = _temporal_desc(params)
    out = np.zeros((h, w), dtype=abi.HISTORY_DTYPE)
    c = ctx.h if ctx else None
    check(lib().yk_history_reproject(c, C.byref(d), _p(history), _p(prev_guides), C.byref(prev_camera.matrices), _p(guides), w, h, _p(out)), c)
    return out


# --------------------------------------------------------------------------- motion (csrc/yk_motion.h)
# After Scene.update the film survives like this — the caller keeps the array it gave to the previous update (or to
# creation), the scene copies what it is given:
#   scene.update(new); guides, ids = render_guides_ids(...); motion = surface_motion(scene, ids, guides, old);
#   carried = reproject_history_moved(history, prev_guides, prev_camera, guides, motion, params); then blend_history,
#   denoise and the tone map as after a camera move.
def render_guides_ids(ctx, scene, camera, film_settings):
    """yk_render_guides_ids: render_guides with the identity of every first hit beside it, from the same single trace ->
    (guides, ids): (h, w) abi.GUIDE_DTYPE, byte for byte render_guides', and (h, w) abi.SURFACE_ID_DTYPE records (shape, b);
    a miss has shape abi.SURFACE_NONE."""
    w, h = film_settings.res
    guides = np.zeros((h, w), dtype=abi.GUIDE_DTYPE)
    ids = np.zeros((h, w), dtype=abi.SURFACE_ID_DTYPE)
    check(lib().yk_render_guides_ids(ctx.h, scene.h, C.byref(camera.matrices), w, h, _p(guides), _p(ids)), ctx.h)
    return guides, ids


def render_guides_through(ctx, scene, camera, film_settings, max_through=4):
    """yk_render_guides_through (csrc/yk_guides_through.h): render_guides_ids' records of the surface every pixel SHOWS —
    glass is followed (transmission; reflection on total internal reflection or a black Kt) for up to max_through
    (0 .. abi.GUIDES_THROUGH_MAX) interfaces -> (guides, ids, through): the (h, w) records of render_guides_ids at the
    first hit that is not glass, and (h, w) uint32, the interfaces crossed.  max_through = 0 is render_guides_ids."""
    w, h = film_settings.res
    guides = np.zeros((h, w), dtype=abi.GUIDE_DTYPE)
    ids = np.zeros((h, w), dtype=abi.SURFACE_ID_DTYPE)
    through = np.zeros((h, w), dtype=np.uint32)
    check(lib().yk_render_guides_through(ctx.h, scene.h, C.byref(camera.matrices), w, h, int(max_through), _p(guides), _p(ids), _p(through)), ctx.h)
    return guides, ids, through


def _prev_points(scene, prev_points):
    nv = int(scene.data.points.shape[0])
    a = np.asarray(prev_points)
    if a.dtype != np.float32:
        raise ValueError(f"prev_points is float32, not {a.dtype}")
    if a.shape not in ((nv, 3), (3 * nv,)):
        raise ValueError(f"prev_points has shape {a.shape}, the scene {nv} vertices: ({nv}, 3)")
    return np.ascontiguousarray(a)


_AT_REST = object()  # surface_motion(prev_transforms=): not given.  None is a value: the scene stood at rest


def _prev_spheres(scene, prev_spheres):
    if not isinstance(prev_spheres, np.ndarray):
        prev_spheres = abi.pack_spheres(prev_spheres)
    if prev_spheres.dtype != abi.SPHERE_DTYPE or prev_spheres.shape != (len(scene.data.spheres),):
        raise ValueError(f"prev_spheres is ({len(scene.data.spheres)},) abi.SPHERE_DTYPE records, not {prev_spheres.shape} {prev_spheres.dtype}")
    return np.ascontiguousarray(prev_spheres)


def _motion_transforms(scene, ids, guides, prev_transforms, prev_spheres, w, h, c):
    n_meshes = len(scene.data.meshes)
    if prev_transforms is not None:
        if not (isinstance(prev_transforms, np.ndarray) and prev_transforms.dtype == abi.MESH_TRANSFORM_DTYPE):
            prev_transforms = abi.pack_mesh_transforms(prev_transforms)
        if prev_transforms.shape != (n_meshes,):
            raise ValueError(f"prev_transforms: {prev_transforms.shape} records, the scene has {n_meshes} meshes")
        prev_transforms = np.ascontiguousarray(prev_transforms)
    if prev_spheres is not None:
        prev_spheres = _prev_spheres(scene, prev_spheres)
    out = np.zeros((h, w), dtype=abi.MOTION_DTYPE)
    check(lib().yk_surface_motion_transforms(c, scene.h, _p(ids), _p(guides), _p(prev_transforms), _p(prev_spheres), w, h, _p(out)), c)
    return out


def surface_motion(scene, ids, guides, prev_points=None, ctx=None, prev_spheres=None, prev_transforms=_AT_REST):
    """yk_surface_motion: where every pixel's surface point stood when the scene's vertices were `prev_points`
    ((n_vertices, 3) float32, the array given to the previous update or to creation) -> (h, w) abi.MOTION_DTYPE records
    (p_prev, known).  `ids` and `guides` are render_guides_ids' of the current geometry.  ctx None = the host instance.
    With `prev_spheres` — the scene's spheres as they were before the last Scene.edit: a list of SceneData spheres or
    (n_spheres,) abi.SPHERE_DTYPE records — yk_surface_motion_spheres: a moved sphere carries its points along;
    `prev_points` may then be None for a scene without triangles.
    With `prev_transforms` instead of prev_points — what the previous Scene.transform got (the same forms), or None: the
    scene stood at rest — yk_surface_motion_transforms: the previous vertices are made of the scene's rest pose and the
    previous matrices, 128 bytes a mesh kept instead of 12 bytes a vertex."""
    guides = np.ascontiguousarray(guides, dtype=abi.GUIDE_DTYPE)
    if guides.ndim != 2:
        raise ValueError("guides is (h, w)")
    h, w = guides.shape
    ids = _records(ids, abi.SURFACE_ID_DTYPE, (w, h), "surface id")
    if prev_transforms is not _AT_REST:
        if prev_points is not None:
            raise ValueError("prev_points and prev_transforms are two ways to say where the vertices stood: give one")
        return _motion_transforms(scene, ids, guides, prev_transforms, prev_spheres, w, h, ctx.h if ctx else None)
    if prev_points is not None or prev_spheres is None:
        prev_points = _prev_points(scene, prev_points)
    out = np.zeros((h, w), dtype=abi.MOTION_DTYPE)
    c = ctx.h if ctx else None
    if prev_spheres is None:
        check(lib().yk_surface_motion(c, scene.h, _p(ids), _p(guides), _p(prev_points), w, h, _p(out)), c)
        return out
    if not isinstance(prev_spheres, np.ndarray):
        prev_spheres = abi.pack_spheres(prev_spheres)
    if prev_spheres.dtype != abi.SPHERE_DTYPE or prev_spheres.shape != (len(scene.data.spheres),):
        raise ValueError(f"prev_spheres is ({len(scene.data.spheres)},) abi.SPHERE_DTYPE records, not {prev_spheres.shape} {prev_spheres.dtype}")
    prev_spheres = np.ascontiguousarray(prev_spheres)
    check(lib().yk_surface_motion_spheres(c, scene.h, _p(ids), _p(guides), _p(prev_points), _p(prev_spheres), w, h, _p(out)), c)
    return out


def surface_albedo(scene, ids, ctx=None):
    """yk_surface_albedo: the diffuse albedo of every pixel's first hit from render_guides_ids' (h, w) `ids` -> (h, w)
    abi.ALBEDO_DTYPE records (a, known): Kd or the texel of a matte surface, (1, 1, 1, 0) for everything denoise(albedo=...)
    is not to demodulate (csrc/yk_albedo.h).  ctx None = the host instance."""
    ids = np.ascontiguousarray(ids, dtype=abi.SURFACE_ID_DTYPE)
    if ids.ndim != 2:
        raise ValueError("ids is (h, w)")
    h, w = ids.shape
    out = np.zeros((h, w), dtype=abi.ALBEDO_DTYPE)
    c = ctx.h if ctx else None
    check(lib().yk_surface_albedo(c, scene.h, _p(ids), w, h, _p(out)), c)
    return out


def _mean_s(s):
    s = int(s)
    if not 1 <= s <= abi.ALBEDO_MEAN_MAX_S:
        raise ValueError(f"s is 1 .. {abi.ALBEDO_MEAN_MAX_S}, not {s}")
    return s


def albedo_mean(scene, ids_ss, s, ctx=None):
    """yk_albedo_mean: the pixel-mean albedo.  `ids_ss` is render_guides_ids' (s * h, s * w) ids of the s-times larger film
    of the same view -> (h, w) abi.ALBEDO_DTYPE records: per channel the float32 mean of surface_albedo's records over every
    pixel's s x s block, known = 1 where any of them is known (csrc/yk_albedo.h).  Every consumer of surface_albedo's
    records takes them.  ctx None = the host instance."""
    s = _mean_s(s)
    ids_ss = np.ascontiguousarray(ids_ss, dtype=abi.SURFACE_ID_DTYPE)
    if ids_ss.ndim != 2 or ids_ss.shape[0] % s or ids_ss.shape[1] % s or ids_ss.size == 0:
        raise ValueError("ids_ss is (s * h, s * w)")
    h, w = ids_ss.shape[0] // s, ids_ss.shape[1] // s
    out = np.zeros((h, w), dtype=abi.ALBEDO_DTYPE)
    c = ctx.h if ctx else None
    check(lib().yk_albedo_mean(c, scene.h, _p(ids_ss), w, h, s, _p(out)), c)
    return out


def supersampled(film_settings, s):
    """The FilmSettings of the s-times larger film of the same view: the film whose pixel centres are the sub-pixel rays of
    albedo_mean."""
    s = _mean_s(s)
    w, h = film_settings.res
    if s * w > 65535 or s * h > 65535:
        raise ValueError(f"s * res = {(s * w, s * h)} exceeds 65535")
    return FilmSettings(res=(s * w, s * h), tile_dim=film_settings.tile_dim)


def render_albedo_mean(ctx, scene, camera_params, film_settings, s=2):
    """yk_render_albedo_mean: albedo_mean of the s-times larger film's ids, traced and reduced on the device in bands of rows
    (the large film never exists) -> (h, w) abi.ALBEDO_DTYPE records, bit for bit albedo_mean(render_guides_ids(...)[1]) at
    the large resolution.  `camera_params` is the camera description Camera takes; the s-times larger camera is built here."""
    w, h = film_settings.res
    cam_ss = Camera(camera_params, supersampled(film_settings, s))
    out = np.zeros((h, w), dtype=abi.ALBEDO_DTYPE)
    check(lib().yk_render_albedo_mean(ctx.h, scene.h, C.byref(cam_ss.matrices), w, h, int(s), _p(out)), ctx.h)
    return out


# --------------------------------------------------------------------------- guided upsampling (csrc/yk_upsample.h)
# A frame sooner: render the film of subsampled(settings, s), its guides, and at FULL resolution the guides and ids alone —
#   low = the film of Camera(params, subsampled(fs, s)); low_guides = render_guides(...) of that camera;
#   guides, ids = render_guides_ids(...) of the full camera; albedo = surface_albedo(scene, ids);
#   low_albedo = albedo_mean(scene, ids, s); low = denoise(low, low_guides, ..., albedo=low_albedo);
#   full = upsample(low, low_guides, guides, UpsampleParams.for_scene(scene, s), low_albedo=low_albedo, albedo=albedo);
# then the tone map as after a full-resolution denoise.
@dataclass
class UpsampleParams:
    """yk_upsample_desc: the factor s (1 .. 8) and the normal and plane-distance stops of csrc/yk_upsample.h, which are
    yk_denoise's; float("inf") switches a stop off.  sigma_plane is in scene units: None stands for "no plane stop" (+inf);
    UpsampleParams.for_scene scales it to the scene."""

    s: int = 2
    sigma_normal: float = 0.3
    sigma_plane: float = None

    @staticmethod
    def for_scene(scene, s, **kw):
        """DenoiseParams.for_scene's stops: sigma_plane = 0.01 x the diagonal of the scene's bounds, sigma_normal 0.3."""
        d = DenoiseParams.for_scene(scene)
        return UpsampleParams(**{**dict(s=s, sigma_normal=d.sigma_normal, sigma_plane=d.sigma_plane), **kw})

    def as_struct(self):
        return abi.UpsampleDesc(int(self.s), float(self.sigma_normal), float("inf") if self.sigma_plane is None else float(self.sigma_plane))


def _upsample_desc(params):
    if not isinstance(params, UpsampleParams):
        raise TypeError("params is an UpsampleParams")
    if not 1 <= int(params.s) <= abi.UPSAMPLE_MAX_S:
        raise ValueError(f"s is 1 .. {abi.UPSAMPLE_MAX_S}, not {params.s}")
    return params.as_struct()


def subsampled(film_settings, s):
    """The FilmSettings of the s-times smaller film of the same view, the inverse of supersampled: the film whose pixels
    each cover an s x s block of this one's.  Raises unless s divides both sides."""
    s = _mean_s(s)
    w, h = film_settings.res
    if w % s or h % s or w < s or h < s:
        raise ValueError(f"s = {s} does not divide res = {(w, h)}")
    return FilmSettings(res=(w // s, h // s), tile_dim=film_settings.tile_dim)


def upsample(low_film, low_guides, guides, params, tile_dim=16, samples=None, low_albedo=None, albedo=None, ctx=None, return_weight=False):
    """yk_upsample: an (lh, lw, 3) float32 film of subsampled(...) rebuilt at (s * lh, s * lw) through its own (lh, lw) guides
    and the full film's (s * lh, s * lw) guides (csrc/yk_upsample.h).  `samples` / `tile_dim` = the LOW film's sample table
    (film_samples), whose sums are normalised first.  low_albedo (albedo_mean(scene, ids, s) of the full ids) and albedo
    (surface_albedo of the full ids) are given both — the upsample then runs on radiance / albedo and multiplies the full
    albedo back — or neither.  Returns the full film; with return_weight also the (s * lh, s * lw) float32 weight sums, 0
    exactly where no tap was taken and the containing low pixel was copied.  ctx None = the host instance."""
    low_film, lw, lh = _film(low_film)
    d = _upsample_desc(params)
    s = int(d.s)
    samples = _blend_samples((lw, lh), tile_dim, samples)
    low_guides = _records(low_guides, abi.GUIDE_DTYPE, (lw, lh), "low guide")
    guides = _records(guides, abi.GUIDE_DTYPE, (s * lw, s * lh), "guide")
    if (low_albedo is None) != (albedo is None):
        raise ValueError("low_albedo and albedo are given both or neither")
    if albedo is not None:
        low_albedo = _records(low_albedo, abi.ALBEDO_DTYPE, (lw, lh), "low albedo")
        albedo = _records(albedo, abi.ALBEDO_DTYPE, (s * lw, s * lh), "albedo")
    out = np.empty((s * lh, s * lw, 3), np.float32)
    weight = np.empty((s * lh, s * lw), np.float32) if return_weight else None
    c = ctx.h if ctx else None
    check(lib().yk_upsample(c, C.byref(d), _p(low_film), _p(low_guides), _p(low_albedo), lw, lh, int(tile_dim), _p(samples), _p(guides), _p(albedo), _p(out), _p(weight)), c)
    return (out, weight) if return_weight else out


def reproject_history_moved(history, prev_guides, prev_camera, guides, motion, params, ctx=None):
    """yk_history_reproject_moved: reproject_history after the geometry moved: every pixel is carried from where its
    surface point stood (`motion`, surface_motion's records) instead of from where it stands.  ctx None = the host
    instance."""
    guides = np.ascontiguousarray(guides, dtype=abi.GUIDE_DTYPE)
    if guides.ndim != 2:
        raise ValueError("guides is (h, w)")
    h, w = guides.shape
    history = _records(history, abi.HISTORY_DTYPE, (w, h), "history")
    prev_guides = _records(prev_guides, abi.GUIDE_DTYPE, (w, h), "guide")
    motion = _records(motion, abi.MOTION_DTYPE, (w, h), "motion")
    d = _temporal_desc(params)
    out = np.zeros((h, w), dtype=abi.HISTORY_DTYPE)
    c = ctx.h if ctx else None
    check(lib().yk_history_reproject_moved(c, C.byref(d), _p(history), _p(prev_guides), C.byref(prev_camera.matrices), _p(guides), _p(motion), w, h, _p(out)), c)
    return out


def _blend_samples(res, tile_dim, samples):
    if samples is not None:
        samples = np.ascontiguousarray(samples, dtype=np.uint32)
        if int(tile_dim) > 0 and samples.size != _table_len(res, int(tile_dim)):
            raise ValueError(f"samples has {samples.size} entries, the film's tile grid {_table_len(res, int(tile_dim))}")
    return samples


def blend_history(film, params, tile_dim=16, samples=None, history=None, ctx=None):
    """yk_history_blend: the current view's (h, w, 3) float32 film (with `samples` = Film.samples for an accumulating one)
    folded into a reprojected history (or None) -> (rgb, history): the film of the means, which downstream passes take with
    samples=None, and the new (h, w) abi.HISTORY_DTYPE history.  ctx None = the host instance."""
    film, w, h = _film(film)
    d = _temporal_desc(params)
    samples = _blend_samples((w, h), tile_dim, samples)
    if history is not None:
        history = _records(history, abi.HISTORY_DTYPE, (w, h), "history")
    rgb = np.empty_like(film)
    out = np.zeros((h, w), dtype=abi.HISTORY_DTYPE)
    c = ctx.h if ctx else None
    check(lib().yk_history_blend(c, C.byref(d), _p(film), w, h, int(tile_dim), _p(samples), _p(history), _p(out), _p(rgb)), c)
    return rgb, out


# --------------------------------------------------------------------------- variance (csrc/yk_variance.h)
# Per frame: render the pass into a cleared film; rgb, history = blend_history(film, tp, samples=..., history=carried);
# moments = blend_moments(film, tp, samples=..., moments=carried_moments) from the SAME film; after a move the moments go
# through reproject_history[_moved] like the history (same layout: pass moments.view(abi.HISTORY_DTYPE));
# var = variance(moments, rgb, guides, vp); out = denoise(rgb, guides, vp, variance=var).
@dataclass
class VarianceParams:
    """yk_variance_desc: the à-trous iterations (0 .. 8), the variance-scaled colour stop, the normal and plane-distance
    stops of DenoiseParams, epsilon under the colour stop and the factor on the spatial estimate (csrc/yk_variance.h);
    float("inf") switches a stop off.  The defaults of sigma_variance, epsilon and spatial_scale are the best row of
    profiles/variance_quality.json.  sigma_plane None stands for "no plane stop"; for_scene scales it to the scene."""

    iterations: int = 5
    sigma_variance: float = 3.0
    sigma_normal: float = 0.3
    sigma_plane: float = None
    epsilon: float = 1e-8
    spatial_scale: float = 1.0

    @staticmethod
    def for_scene(scene, **kw):
        """sigma_plane = 0.01 x the diagonal of the scene's bounds (Scene.info()), as DenoiseParams.for_scene."""
        return VarianceParams(sigma_plane=0.01 * _scene_diagonal(scene), **kw)

    def as_struct(self):
        return abi.VarianceDesc(int(self.iterations), float(self.sigma_variance), float(self.sigma_normal), float("inf") if self.sigma_plane is None else float(self.sigma_plane), float(self.epsilon), float(self.spatial_scale))


def _variance_desc(params):
    if not isinstance(params, VarianceParams):
        raise TypeError("params is a VarianceParams")
    return params.as_struct()


def blend_moments(film, params, tile_dim=16, samples=None, moments=None, ctx=None):
    """yk_moments_blend: the luminance of the film blend_history folds into the history, folded into the (reprojected)
    (h, w) abi.MOMENTS_DTYPE moments (or None) -> the new moments.  `params` is blend_history's TemporalParams.  ctx None =
    the host instance."""
    film, w, h = _film(film)
    d = _temporal_desc(params)
    samples = _blend_samples((w, h), tile_dim, samples)
    if moments is not None:
        moments = _records(moments, abi.MOMENTS_DTYPE, (w, h), "moments")
    out = np.zeros((h, w), dtype=abi.MOMENTS_DTYPE)
    c = ctx.h if ctx else None
    check(lib().yk_moments_blend(c, C.byref(d), _p(film), w, h, int(tile_dim), _p(samples), _p(moments), _p(out)), c)
    return out


def variance(moments, film, guides, params, tile_dim=16, samples=None, ctx=None, albedo=None):
    """yk_variance: the (h, w) float32 variance of the luminance of `film` as denoise(..., variance=) will filter it: from
    the moments (or None) where they hold two frames or more, from the 7 x 7 neighbourhood everywhere else.  With albedo:
    the variance of the demodulated film.  ctx None = the host instance."""
    film, w, h = _film(film)
    d = _variance_desc(params)
    samples = _blend_samples((w, h), tile_dim, samples)
    guides = _records(guides, abi.GUIDE_DTYPE, (w, h), "guide")
    if moments is not None:
        moments = _records(moments, abi.MOMENTS_DTYPE, (w, h), "moments")
    if albedo is not None:
        albedo = _records(albedo, abi.ALBEDO_DTYPE, (w, h), "albedo")
    out = np.zeros((h, w), dtype=np.float32)
    c = ctx.h if ctx else None
    check(lib().yk_variance(c, C.byref(d), _p(moments), _p(film), _p(guides), _p(albedo), w, h, int(tile_dim), _p(samples), _p(out)), c)
    return out


# --------------------------------------------------------------------------- rectification (csrc/yk_rectify.h)
# Per frame, before the blends: history = rectify_history(carried, film, rp, samples=...) — carried being the reprojected
# history after a move and the last blend's history while the view stands — or, with moments,
# history, moments = rectify_history(carried, film, rp, samples=..., moments=carried_moments); then blend_history and
# blend_moments from the same film.
@dataclass
class RectifyParams:
    """yk_rectify_desc: the window is (2 radius + 1)^2 pixels of the current film (radius 1 .. 3), the box mean +- gamma
    standard deviations per channel (gamma >= 0; float("inf") lets every history through).  The defaults are the best row
    of profiles/rectify_quality.json."""

    radius: int = 2
    gamma: float = 0.75

    def as_struct(self):
        return abi.RectifyDesc(int(self.radius), float(self.gamma))


def _rectify_desc(params):
    if not isinstance(params, RectifyParams):
        raise TypeError("params is a RectifyParams")
    return params.as_struct()


def rectify_history(history, film, params, tile_dim=16, samples=None, moments=None, ctx=None):
    """yk_history_rectify: the carried (h, w) abi.HISTORY_DTYPE history clipped to the box of the current view's (h, w, 3)
    float32 film (with `samples` = Film.samples for an accumulating one, as blend_history takes it) -> the history for
    blend_history; with the (h, w) abi.MOMENTS_DTYPE moments beside it -> (history, moments).  ctx None = the host
    instance."""
    film, w, h = _film(film)
    d = _rectify_desc(params)
    samples = _blend_samples((w, h), tile_dim, samples)
    history = _records(history, abi.HISTORY_DTYPE, (w, h), "history")
    out = np.zeros((h, w), dtype=abi.HISTORY_DTYPE)
    out_m = None
    if moments is not None:
        moments = _records(moments, abi.MOMENTS_DTYPE, (w, h), "moments")
        out_m = np.zeros((h, w), dtype=abi.MOMENTS_DTYPE)
    c = ctx.h if ctx else None
    check(lib().yk_history_rectify(c, C.byref(d), _p(film), w, h, int(tile_dim), _p(samples), _p(history), _p(moments), _p(out), _p(out_m)), c)
    return out if moments is None else (out, out_m)


# --------------------------------------------------------------------------- despeckle (csrc/yk_despeckle.h)
# Per frame, first: film = despeckle(film, dp, samples=...) on the current frame's film — the output keeps the input's
# convention, so the same sample table goes on with it — then rectify_history, blend_history, blend_moments as above.
@dataclass
class DespeckleParams:
    """yk_despeckle_desc: a pixel brighter than gain x the rank-th largest luminance among the other pixels of its
    (2 radius + 1)^2 window (radius 1 .. 2, rank 1 .. 4) is scaled down to that bound; with fewer than max(min_taps, rank)
    usable neighbours, or below the luminance `floor`, it is left alone; repair replaces a pixel that is not finite by the
    mean of its usable neighbours.  gain float("inf") clamps nothing.  The defaults of radius, rank and gain are the best
    row of profiles/despeckle_quality.json.  Biased by design: not for a film meant to converge."""

    radius: int = 2
    rank: int = 3
    gain: float = 1.5
    min_taps: int = 3
    floor: float = 0.0
    repair: bool = False

    def as_struct(self):
        return abi.DespeckleDesc(int(self.radius), int(self.rank), int(self.min_taps), abi.DESPECKLE_REPAIR if self.repair else 0, float(self.gain), float(self.floor))


def _despeckle_desc(params):
    if not isinstance(params, DespeckleParams):
        raise TypeError("params is a DespeckleParams")
    return params.as_struct()


def despeckle(film, params, tile_dim=16, samples=None, ctx=None, return_mask=False):
    """yk_despeckle: the (h, w, 3) float32 film (with `samples` = Film.samples for an accumulating one, as blend_history
    takes it) with its outliers clamped -> the film, in the input's convention (a film of sums stays one).  With
    return_mask: (film, mask, counts) — the (h, w) uint8 mask (0 untouched, 1 clamped, 2 repaired) and the two counts
    (clamped, repaired).  ctx None = the host instance."""
    film, w, h = _film(film)
    d = _despeckle_desc(params)
    samples = _blend_samples((w, h), tile_dim, samples)
    out = np.empty_like(film)
    mask = np.zeros((h, w), dtype=np.uint8) if return_mask else None
    counts = np.zeros(2, dtype=np.uint32) if return_mask else None
    c = ctx.h if ctx else None
    check(lib().yk_despeckle(c, C.byref(d), _p(film), w, h, int(tile_dim), _p(samples), _p(out), _p(mask), _p(counts)), c)
    return (out, mask, (int(counts[0]), int(counts[1]))) if return_mask else out


def _despeckle_for_output(film, despeckle_params, tile_dim, samples, ctx):
    """The despeckle step of write_output / write_preview, before the denoise: None leaves the film as it is."""
    if despeckle_params is None:
        return film
    return despeckle(film, despeckle_params, tile_dim, samples, ctx)


# --------------------------------------------------------------------------- adaptive sampling (csrc/yk_adaptive.h)
# film_sum (h, w, 3) float32 sums and stats (h, w) abi.PIXEL_STATS_DTYPE, both zeros when cleared.  Per round:
# xy, sample = adaptive_select(stats, params); passes = the render of those entries (Integrator.render_pixel_list_device);
# adaptive_accumulate(xy, passes, film_sum, stats).  At the end rgb, var = adaptive_resolve(film_sum, stats) and
# denoise(rgb, guides, VarianceParams, variance=var).  Integrator.render_adaptive is that loop on the device.
@dataclass
class AdaptiveParams:
    """yk_adaptive_desc (csrc/yk_adaptive.h): a pixel wants samples while it has fewer than min_samples or the standard
    error of its mean luminance exceeds threshold x (mean + epsilon); with dilate its 8 neighbours are taken along; a
    selected pixel takes round_passes samples a round and never more than max_samples in all; max_rounds 0 = until nothing
    is selected.  The defaults are the best row of profiles/adaptive_quality.json; max_samples None stands for "the
    sampler's samples per pixel" (for_sampler)."""

    min_samples: int = 16
    max_samples: int = None
    round_passes: int = 8
    max_rounds: int = 0
    dilate: bool = True
    threshold: float = 0.2
    epsilon: float = 0.05

    @staticmethod
    def for_sampler(sampler, **kw):
        """max_samples = the sampler's samples per pixel: the most a pixel can take."""
        return AdaptiveParams(max_samples=samples_per_pixel(sampler), **kw)

    def as_struct(self):
        if self.max_samples is None:
            raise ValueError("AdaptiveParams.max_samples is not set: use AdaptiveParams.for_sampler")
        return abi.AdaptiveDesc(int(self.min_samples), int(self.max_samples), int(self.round_passes), int(self.max_rounds), int(self.dilate), float(self.threshold), float(self.epsilon))


def _adaptive_desc(params):
    if not isinstance(params, AdaptiveParams):
        raise TypeError("params is an AdaptiveParams")
    return params.as_struct()


def _film_sum(film_sum):
    if film_sum.dtype != np.float32 or not film_sum.flags.c_contiguous or film_sum.ndim != 3 or film_sum.shape[2] != 3:
        raise ValueError("film_sum is a contiguous (h, w, 3) float32 array")
    return film_sum.shape[1], film_sum.shape[0]


def adaptive_select(stats, params, ctx=None):
    """yk_adaptive_select: the (h, w) abi.PIXEL_STATS_DTYPE statistics -> (xy, sample), two uint32 arrays with one entry per
    selected pixel in the rule's order (xy = x | y << 16, sample = the pixel's next sample index).  ctx None = the host
    instance."""
    if stats.ndim != 2:
        raise ValueError("stats is (h, w)")
    h, w = stats.shape
    stats = _records(stats, abi.PIXEL_STATS_DTYPE, (w, h), "pixel stats")
    d = _adaptive_desc(params)
    xy = np.zeros(w * h, dtype=np.uint32)
    sample = np.zeros(w * h, dtype=np.uint32)
    n = C.c_uint32(0)
    c = ctx.h if ctx else None
    check(lib().yk_adaptive_select(c, C.byref(d), _p(stats), w, h, _p(xy), _p(sample), C.byref(n)), c)
    return xy[: n.value].copy(), sample[: n.value].copy()


def adaptive_accumulate(xy, passes, film_sum, stats, ctx=None):
    """yk_adaptive_accumulate: folds passes (n_passes, n, 3) — entry e's values in pass order — into film_sum and stats IN
    PLACE at the pixels xy names.  ctx None = the host instance."""
    w, h = _film_sum(film_sum)
    if stats.dtype != abi.PIXEL_STATS_DTYPE or not stats.flags.c_contiguous or stats.shape != (h, w):
        raise ValueError("stats is a contiguous (h, w) array of abi.PIXEL_STATS_DTYPE")
    xy = np.ascontiguousarray(xy, dtype=np.uint32)
    passes = np.ascontiguousarray(passes, dtype=np.float32)
    if passes.ndim != 3 or passes.shape[1] != len(xy) or passes.shape[2] != 3:
        raise ValueError("passes is (n_passes, n, 3)")
    c = ctx.h if ctx else None
    check(lib().yk_adaptive_accumulate(c, _p(xy), len(xy), _p(passes), passes.shape[0], w, h, _p(film_sum), _p(stats)), c)


def adaptive_resolve(film_sum, stats, ctx=None):
    """yk_adaptive_resolve: (rgb (h, w, 3), variance (h, w)) — the mean film and the variance of that mean, the image
    denoise(..., variance=) takes.  ctx None = the host instance."""
    film_sum = np.ascontiguousarray(film_sum, dtype=np.float32)
    w, h = _film_sum(film_sum)
    stats = _records(stats, abi.PIXEL_STATS_DTYPE, (w, h), "pixel stats")
    rgb = np.zeros((h, w, 3), dtype=np.float32)
    var = np.zeros((h, w), dtype=np.float32)
    c = ctx.h if ctx else None
    check(lib().yk_adaptive_resolve(c, _p(film_sum), _p(stats), w, h, _p(rgb), _p(var)), c)
    return rgb, var


def _denoise_for_output(film, denoise_params, guides, tile_dim, samples, ctx, albedo=None, variance=None):
    """The denoise step of write_output / write_preview: (film, samples) for the tone map that follows — the denoised film
    is normalised already, so it goes on without the sample table."""
    if denoise_params is None:
        if albedo is not None or variance is not None:
            raise ValueError("albedo and variance need denoise (a DenoiseParams or VarianceParams) and guides")
        return film, samples
    if guides is None:
        raise ValueError("denoise needs guides (render_guides)")
    return denoise(film, guides, denoise_params, tile_dim, samples, ctx, albedo, variance), None


def _guides_through_for_output(guides_through, settings, ctx, guides, albedo):
    """The guides_through= keyword of write_output / write_preview: (scene, camera) or (scene, camera, max_through) — the
    guides are rendered here by render_guides_through on `ctx` instead of being passed in, and albedo=True asks for
    surface_albedo of the same call's ids.  -> (guides, albedo)."""
    if guides_through is None:
        if albedo is True:
            raise ValueError("albedo=True needs guides_through: the ids come from its call")
        return guides, albedo
    if guides is not None:
        raise ValueError("guides_through renders the guides: pass one of the two")
    if ctx is None:
        raise ValueError("guides_through renders on the device: it needs ctx")
    scene, camera = guides_through[0], guides_through[1]
    max_through = guides_through[2] if len(guides_through) > 2 else 4
    guides, ids, _ = render_guides_through(ctx, scene, camera, settings, max_through)
    if albedo is True:
        albedo = surface_albedo(scene, ids, ctx)
    return guides, albedo


def write_output(path, film, tone_map=None, settings=None, samples=None, ctx=None, denoise=None, guides=None, albedo=None, variance=None, auto_exposure=None, guides_through=None, despeckle=None):
    """The Finished branch of app/headless.rs:62-84: Raw writes the film as it is, anything else writes the tone-mapped
    film (a Heatmap without bounds finds them first).  tone_map None = ToneMapType.default(); settings None = a film of the
    array's size with the default tile_dim.  denoise (a DenoiseParams) with guides: the film is denoised first; with albedo
    (surface_albedo's records) too: by the demodulated filter; with a VarianceParams and variance (variance()'s image): by
    the variance-guided filter.  auto_exposure (True or an ExposureParams, Filmic only): the film about to be tone-mapped
    — after the denoise — is metered (meter_exposure) and the exposure is the tone map's times the meter's.
    guides_through ((scene, camera[, max_through]), instead of guides, with ctx): the guides are render_guides_through's —
    what the pixel shows behind glass — and albedo=True takes surface_albedo of that call's ids.  despeckle (a
    DespeckleParams): the film's outliers are clamped first, before the denoise."""
    film = np.ascontiguousarray(film, dtype=np.float32)
    tone_map = ToneMapType.default() if tone_map is None else tone_map
    settings = settings or FilmSettings(res=(film.shape[1], film.shape[0]))
    film = _despeckle_for_output(film, despeckle, film_tile_dim(settings), samples, ctx)
    guides, albedo = _guides_through_for_output(guides_through, settings, ctx, guides, albedo)
    film, samples = _denoise_for_output(film, denoise, guides, film_tile_dim(settings), samples, ctx, albedo, variance)
    if tone_map.kind == abi.TONE_MAP_RAW:
        if auto_exposure:
            raise ValueError("auto_exposure needs the Filmic tone map: the others have no exposure")
        write_exr(path, film)
        return
    tone_map = _auto_exposure(film, tone_map, auto_exposure, film_tile_dim(settings), samples, ctx)
    write_exr(path, _apply_tone_map(film, tone_map, film_tile_dim(settings), samples, ctx, None))


# --------------------------------------------------------------------------- overlays
def _camera_params(params, res):
    if isinstance(params, dict):
        params = CameraParameters(**params)
    p = abi.CameraParams()
    p.position = abi.f3(params.position)
    p.target = abi.f3(params.target)
    p.up = abi.f3(params.up)
    p.fov_axis = params.fov_axis
    p.fov_degrees = params.fov_degrees
    p.res_x, p.res_y = res
    return p


def overlay_world_to_clip(camera_params, film_settings, scene_bounds):
    """The `world_to_clip` of RayVisualization::draw / BvhVisualization::draw (ray_visualization.rs:80-150): (4, 4) float32,
    row-major.  scene_bounds: (p_min, p_max) of scene.bvh.bounds(), e.g. Scene.node_bounds(0)[0]."""
    p = _camera_params(camera_params, film_settings.res)
    bounds = np.ascontiguousarray(scene_bounds, dtype=np.float32).reshape(6)
    out = np.zeros((4, 4), dtype=np.float32)
    check(lib().yk_overlay_world_to_clip(C.byref(p), _p(bounds), _p(out)))
    return out


def overlay_ray_lines(rays):
    """RayVisualization::set_rays (ray_visualization.rs:28-56): li_debug records (abi.INTEGRATOR_RAY_DTYPE) -> lines
    (abi.OVERLAY_LINE_DTYPE) coloured by ray type."""
    rays = np.ascontiguousarray(rays, dtype=abi.INTEGRATOR_RAY_DTYPE).reshape(-1)
    out = np.zeros(len(rays), dtype=abi.OVERLAY_LINE_DTYPE)
    check(lib().yk_overlay_ray_lines(_p(rays), len(rays), _p(out)))
    return out


def _overlay_args(world_to_clip, lines, boxes):
    m = np.ascontiguousarray(world_to_clip, dtype=np.float32).reshape(16)
    lines = None if lines is None else np.ascontiguousarray(lines, dtype=abi.OVERLAY_LINE_DTYPE).reshape(-1)
    boxes = None if boxes is None else np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 6)
    return m, lines, boxes


def draw_overlay(film, world_to_clip, lines=None, boxes=None, ctx=None):
    """yk_overlay_draw: the lines, then the boxes ((n, 2, 3) or (n, 6): p_min, p_max), drawn into a copy of the
    (h, w, 3) float32 film by the rule of csrc/yk_overlay.h.  ctx None = the host instance."""
    out = np.array(film, dtype=np.float32, order="C", copy=True)
    m, lines, boxes = _overlay_args(world_to_clip, lines, boxes)
    c = ctx.h if ctx else None
    check(lib().yk_overlay_draw(c, _p(m), _p(lines), 0 if lines is None else len(lines), _p(boxes), 0 if boxes is None else len(boxes), _p(out), out.shape[1], out.shape[0]), c)
    return out


def draw_visualizations(film, scene, camera_params, film_settings, rays=None, bvh_level=None, ctx=None):
    """draw_visualizations (app/window.rs:1033-1063) on a tone-mapped (h, w, 3) film: the rays of a debug sample
    (li_debug records, or None), then the boxes of BVH level `bvh_level` (-1 = every level, None = none), both under the
    world_to_clip of the scene's root box.  Returns the new film; ctx None = the host instance."""
    m = overlay_world_to_clip(camera_params, film_settings, scene.node_bounds(0)[0])
    lines = None if rays is None else overlay_ray_lines(rays)
    boxes = None if bvh_level is None else scene.node_bounds(bvh_level)
    return draw_overlay(film, m, lines, boxes, ctx)


# --------------------------------------------------------------------------- present
_PRESENT_FORMATS = {"rgba8": abi.PRESENT_RGBA8, "rgb32f": abi.PRESENT_RGB32F}


def _present_desc(window, encode, fmt):
    if isinstance(fmt, str):
        if fmt not in _PRESENT_FORMATS:
            raise ValueError(f"fmt is 'rgba8' or 'rgb32f', not {fmt!r}")
        fmt = _PRESENT_FORMATS[fmt]
    return abi.PresentDesc(int(window[0]), int(window[1]), int(encode), int(fmt))


def present_target_rect(res, window):
    """The target rectangle of ScaleOutput::draw (scale_output.rs:64-84) for a film of `res` = (w, h) in a window (W, H):
    (x0, y0, width, height) in top-down window coordinates, unclipped."""
    r = abi.PresentRect()
    check(lib().yk_present_target_rect(int(res[0]), int(res[1]), int(window[0]), int(window[1]), C.byref(r)))
    return int(r.x0), int(r.y0), int(r.width), int(r.height)


def present(film, window, encode=2, fmt="rgba8", ctx=None):
    """ScaleOutput::draw (app/renderpasses/scale_output.rs) by the rule of csrc/yk_present.h: the (h, w, 3) float32
    tone-mapped film stretched into a window (W, H) with bilinear filtering inside a letterbox.  encode 0 none, 1 the
    shader's linearToSRGB, 2 an sRGB back buffer (the reference's default).  Returns (H, W, 4) uint8 for fmt "rgba8",
    (H, W, 3) float32 (the values before quantisation) for "rgb32f".  ctx None = the host instance."""
    film, w, h = _film(film)
    d = _present_desc(window, encode, fmt)
    out = np.empty((d.window_y, d.window_x, 4), dtype=np.uint8) if d.format == abi.PRESENT_RGBA8 else np.empty((d.window_y, d.window_x, 3), dtype=np.float32)
    c = ctx.h if ctx else None
    check(lib().yk_present(c, C.byref(d), _p(film), w, h, _p(out)), c)
    return out


def write_png(path, pixels):
    """yk_write_png: (h, w, 3) or (h, w, 4) uint8 -> an 8-bit PNG, row 0 at the top."""
    pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
    if pixels.ndim != 3:
        raise ValueError("pixels is (h, w, 3) or (h, w, 4)")
    check(lib().yk_write_png(str(path).encode(), pixels.shape[1], pixels.shape[0], pixels.shape[2], _p(pixels)))


def write_preview(path, film, tone_map=None, settings=None, samples=None, window=None, ctx=None, denoise=None, guides=None, albedo=None, variance=None, auto_exposure=None, guides_through=None, despeckle=None):
    """What the window shows, as a PNG: the denoiser when `denoise` (a DenoiseParams) and `guides` are given (demodulated
    by `albedo`, surface_albedo's records, when that is given too; variance-guided when `denoise` is a VarianceParams and
    `variance` its image), the tone map
    (as write_output: None = ToneMapType.default(), Raw = none), then present into `window` (default: the film's size) as
    an sRGB back buffer stores it (encode 2), then write_png.  auto_exposure, guides_through and despeckle: as
    write_output's."""
    film = np.ascontiguousarray(film, dtype=np.float32)
    tone_map = ToneMapType.default() if tone_map is None else tone_map
    settings = settings or FilmSettings(res=(film.shape[1], film.shape[0]))
    film = _despeckle_for_output(film, despeckle, film_tile_dim(settings), samples, ctx)
    guides, albedo = _guides_through_for_output(guides_through, settings, ctx, guides, albedo)
    film, samples = _denoise_for_output(film, denoise, guides, film_tile_dim(settings), samples, ctx, albedo, variance)
    if tone_map.kind != abi.TONE_MAP_RAW:
        tone_map = _auto_exposure(film, tone_map, auto_exposure, film_tile_dim(settings), samples, ctx)
        film = _apply_tone_map(film, tone_map, film_tile_dim(settings), samples, ctx, None)
    elif auto_exposure:
        raise ValueError("auto_exposure needs the Filmic tone map: the others have no exposure")
    window = (film.shape[1], film.shape[0]) if window is None else window
    write_png(path, present(film, window, abi.PRESENT_ENCODE_SRGB, "rgba8", ctx))


class TileList:
    """A tile list prepared once on the device (yk_tile_list): the GPU worker's tile queue."""

    def __init__(self, ctx, tiles, tile_samples=None):
        self.ctx = ctx
        self.tiles = np.ascontiguousarray(tiles, dtype=abi.TILE_DTYPE)
        ts = None if tile_samples is None else np.ascontiguousarray(tile_samples, dtype=np.uint16)
        h = C.c_void_p()
        check(lib().yk_tile_list_create(ctx.h, _p(self.tiles), _p(ts), len(self.tiles), C.byref(h)), ctx.h)
        self.h = h
        self.n_pixels = int(((self.tiles["x1"].astype(np.int64) - self.tiles["x0"]) * (self.tiles["y1"].astype(np.int64) - self.tiles["y0"])).sum())

    def update_film_device(self, d_tile_rgb_ptr, res, d_film_ptr, stream=None, accumulate=False, ctx=None, n_passes=1):
        """Film::update_tile for the whole list, device to device, enqueued on `stream` (default:
        the stream of `ctx`, any context on the list's device; default the one that made it).
        n_passes > 1: `d_tile_rgb_ptr` holds that many passes (pass-major), added one after the other."""
        c = ctx or self.ctx
        if n_passes != 1:
            if not accumulate:
                raise ValueError("several passes only make sense for the accumulating film")
            check(lib().yk_film_accumulate_tile_list_passes_device(c.h, self.h, C.c_void_p(d_tile_rgb_ptr), n_passes, res[0], res[1], C.c_void_p(d_film_ptr), _vp(stream)), c.h)
            return
        check(lib().yk_film_update_tile_list_device(c.h, self.h, C.c_void_p(d_tile_rgb_ptr), res[0], res[1], C.c_void_p(d_film_ptr), _vp(stream), 1 if accumulate else 0), c.h)

    def close(self):
        if getattr(self, "h", None):
            lib().yk_tile_list_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PixelList:
    """(pixel, first sample index) entries on the device with room for every pixel of a film (yk_pixel_list): filled by
    Context.adaptive_select_device or set(), rendered by Integrator.render_pixel_list_device."""

    def __init__(self, ctx, res):
        self.ctx = ctx
        self.res = (int(res[0]), int(res[1]))
        h = C.c_void_p()
        check(lib().yk_pixel_list_create(ctx.h, self.res[0], self.res[1], C.byref(h)), ctx.h)
        self.h = h
        self.n = 0

    def set(self, xy, sample, passes=1):
        """Host entries (xy = x | y << 16), checked before the upload: inside the resolution, no pixel twice."""
        xy = np.ascontiguousarray(xy, dtype=np.uint32)
        sample = np.ascontiguousarray(sample, dtype=np.uint32)
        if xy.shape != sample.shape or xy.ndim != 1:
            raise ValueError("one sample index per entry")
        check(lib().yk_pixel_list_set(self.h, _p(xy), _p(sample), len(xy), int(passes)), self.ctx.h)
        self.n = len(xy)

    def read(self):
        """(xy, sample) as the device holds them."""
        n = C.c_uint32(0)
        check(lib().yk_pixel_list_read(self.h, None, None, 0, C.byref(n)), self.ctx.h)
        xy = np.zeros(n.value, dtype=np.uint32)
        sample = np.zeros(n.value, dtype=np.uint32)
        check(lib().yk_pixel_list_read(self.h, _p(xy), _p(sample), n.value, C.byref(n)), self.ctx.h)
        self.n = n.value
        return xy, sample

    def close(self):
        if getattr(self, "h", None):
            lib().yk_pixel_list_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# --------------------------------------------------------------------------- camera
class FoV:
    X, Y = abi.FOV_X, abi.FOV_Y


@dataclass
class CameraParameters:
    """camera.rs:24-41."""

    position: tuple = (0.0, 0.0, 0.0)
    target: tuple = (0.0, 0.0, 0.0)
    up: tuple = (0.0, 1.0, 0.0)
    fov_axis: int = FoV.X
    fov_degrees: float = 0.0


class Camera:
    """camera.rs:19-22,52-102: built on the host by yk_camera_init."""

    def __init__(self, params, film_settings):
        if isinstance(params, dict):
            params = CameraParameters(**params)
        p = abi.CameraParams()
        p.position = abi.f3(params.position)
        p.target = abi.f3(params.target)
        p.up = abi.f3(params.up)
        p.fov_axis = params.fov_axis
        p.fov_degrees = params.fov_degrees
        p.res_x, p.res_y = film_settings.res
        self.matrices = abi.CameraMatrices()
        check(lib().yk_camera_init(C.byref(p), C.byref(self.matrices)))


# --------------------------------------------------------------------------- sampler / integrator descriptions
class SamplerType:
    """sampling/mod.rs:16-31.  `seed` is explicit (the reference draws it from
    thread_rng(): uniform.rs:37); the default is the reference's commented debug seed."""

    DEBUG_SEED = 0x73B9642E74AC471C

    @staticmethod
    def Uniform(pixel_samples=1, seed=DEBUG_SEED):
        return abi.SamplerDesc(abi.SAMPLER_UNIFORM, pixel_samples, 1, 1, seed)

    @staticmethod
    def Stratified(pixel_samples=(1, 1), jitter_samples=True, seed=DEBUG_SEED):
        return abi.SamplerDesc(abi.SAMPLER_STRATIFIED, pixel_samples[0], pixel_samples[1], 1 if jitter_samples else 0, seed)


def samples_per_pixel(sampler):
    return sampler.nx if sampler.kind == abi.SAMPLER_UNIFORM else sampler.nx * sampler.ny


@dataclass
class PathParams:
    """integrators/path.rs:20-32."""

    max_depth: int = 3
    indirect_clamp: float = None


class LightFactory:
    """RectangularLight::new / SpotLight::new / PointLight::new on the host."""

    @staticmethod
    def make_rect_light(l2w, l2w_inv, L, size, out):
        check(lib().yk_make_rect_light(abi.f16(l2w), abi.f16(l2w_inv), abi.f3(L), (C.c_float * 2)(*[float(s) for s in size]), C.byref(out)))

    @staticmethod
    def make_spot_light(l2w, l2w_inv, I, total, falloff, out):
        check(lib().yk_make_spot_light(abi.f16(l2w), abi.f16(l2w_inv), abi.f3(I), float(total), float(falloff), C.byref(out)))

    @staticmethod
    def make_point_light(l2w, I, out):
        check(lib().yk_make_point_light(abi.f16(l2w), abi.f3(I), C.byref(out)))


# --------------------------------------------------------------------------- context / scene
class Context:
    """One HIP device + stream + work buffers (yk_context)."""

    def __init__(self, device=0, **options):
        h = C.c_void_p()
        check(lib().yk_context_create(device, C.byref(h)))
        self.h = h
        self.device = device
        for k, v in options.items():
            self.set_option(k, v)

    def set_option(self, key, value):
        check(lib().yk_context_set_option(self.h, key.encode(), int(value)), self.h)

    def interrupt(self):
        """yk_context_interrupt: stop what the context has enqueued (any thread)."""
        check(lib().yk_context_interrupt(self.h))

    def tone_map_device(self, d_film_ptr, res, tile_dim, tone_map, samples, d_out_ptr, stream=None, exposure_state=None):
        """yk_tone_map_device: device film -> device out, enqueued on `stream` (default: the context's) without waiting;
        `samples` is a host table (or None), copied before the call returns.  exposure_state: the device pointer of a
        yk_exposure_state (meter_exposure_device's output) — yk_tone_map_metered_device, Filmic only: the exposure is the
        descriptor's times the record's, read on the device when the kernel runs."""
        samples = _tone_map_args(res, tone_map, tile_dim, samples)
        if exposure_state is not None:
            check(lib().yk_tone_map_metered_device(self.h, C.byref(tone_map), _vp(exposure_state), _vp(d_film_ptr), res[0], res[1], int(tile_dim), _p(samples), _vp(d_out_ptr), _vp(stream)), self.h)
            return
        check(lib().yk_tone_map_device(self.h, C.byref(tone_map), _vp(d_film_ptr), res[0], res[1], int(tile_dim), _p(samples), _vp(d_out_ptr), _vp(stream)), self.h)

    def meter_exposure_device(self, d_film_ptr, res, tile_dim, params, samples, d_prev_ptr, d_out_state_ptr, stream=None):
        """yk_exposure_meter_device: the device film's yk_exposure_state (32 bytes, 4-byte aligned) into device memory,
        after the record at d_prev_ptr (None = no history; may be d_out_state_ptr), enqueued on `stream` (default: the
        context's) without waiting.  params None = ExposureParams(); `samples` is a host table (or None)."""
        samples = _tone_map_args(res, ToneMapType.Raw, tile_dim, samples)
        d = (params or ExposureParams()).desc(res)
        check(lib().yk_exposure_meter_device(self.h, C.byref(d), _vp(d_film_ptr), res[0], res[1], int(tile_dim), _p(samples), _vp(d_prev_ptr), _vp(d_out_state_ptr), _vp(stream)), self.h)

    def draw_overlay_device(self, d_film_ptr, res, world_to_clip, d_lines_ptr=None, n_lines=0, d_boxes_ptr=None, n_boxes=0, stream=None):
        """yk_overlay_draw_device: n_lines yk_overlay_line records and n_boxes boxes of six floats, both on the device,
        drawn in place into the device film; enqueued on `stream` (default: the context's) without waiting."""
        m = np.ascontiguousarray(world_to_clip, dtype=np.float32).reshape(16)
        check(
            lib().yk_overlay_draw_device(self.h, _p(m), _vp(d_lines_ptr), int(n_lines), _vp(d_boxes_ptr), int(n_boxes), _vp(d_film_ptr), res[0], res[1], _vp(stream)),
            self.h,
        )

    def present_device(self, d_film_ptr, res, window, encode, fmt, d_out_ptr, stream=None):
        """yk_present_device: the device film of `res` = (w, h) -> the device frame of `window` = (W, H) ("rgba8": 4 bytes
        a pixel, "rgb32f": three floats), enqueued on `stream` (default: the context's) without waiting; one kernel, no
        allocation.  Both pointers need 4-byte alignment."""
        d = _present_desc(window, encode, fmt)
        check(lib().yk_present_device(self.h, C.byref(d), _vp(d_film_ptr), int(res[0]), int(res[1]), _vp(d_out_ptr), _vp(stream)), self.h)

    def render_guides_device(self, scene, camera, res, d_guides_ptr, stream=None):
        """yk_render_guides_device: res[0] * res[1] yk_guide records (32 bytes each, 16-byte aligned) into device memory,
        ordered on `stream` (default: the context's) without waiting on the host."""
        check(lib().yk_render_guides_device(self.h, scene.h, C.byref(camera.matrices), int(res[0]), int(res[1]), _vp(d_guides_ptr), _vp(stream)), self.h)

    def denoise_device(self, d_film_ptr, d_guides_ptr, res, params, tile_dim, samples, d_out_ptr, stream=None, albedo=None):
        """yk_denoise_device: device film + device guides -> device out (may be the film), enqueued on `stream` (default:
        the context's) without waiting; `samples` is a host table (or None), copied before the call returns."""
        d, _, samples = _denoise_args(res, params, None, tile_dim, samples)
        if albedo is not None:  # the device pointer of surface_albedo_device's records: yk_denoise_albedo_device
            check(lib().yk_denoise_albedo_device(self.h, C.byref(d), _vp(d_film_ptr), _vp(d_guides_ptr), _vp(albedo), int(res[0]), int(res[1]), int(tile_dim), _p(samples), _vp(d_out_ptr), _vp(stream)), self.h)
            return
        check(lib().yk_denoise_device(self.h, C.byref(d), _vp(d_film_ptr), _vp(d_guides_ptr), int(res[0]), int(res[1]), int(tile_dim), _p(samples), _vp(d_out_ptr), _vp(stream)), self.h)

    def reproject_history_device(self, d_prev_history_ptr, d_prev_guides_ptr, prev_camera, d_guides_ptr, res, params, d_out_history_ptr, stream=None):
        """yk_history_reproject_device: the previous view's device history and guides, its Camera and the current view's
        device guides -> the device history of the current view (all 16-byte aligned), enqueued on `stream` (default: the
        context's) without waiting."""
        d = _temporal_desc(params)
        check(lib().yk_history_reproject_device(self.h, C.byref(d), _vp(d_prev_history_ptr), _vp(d_prev_guides_ptr), C.byref(prev_camera.matrices), _vp(d_guides_ptr), int(res[0]), int(res[1]), _vp(d_out_history_ptr), _vp(stream)), self.h)

    def render_guides_ids_device(self, scene, camera, res, d_guides_ptr, d_ids_ptr, stream=None):
        """yk_render_guides_ids_device: render_guides_device with res[0] * res[1] yk_surface_id records (16 bytes each,
        16-byte aligned) beside the guides, from the same trace; either pointer may be None, not both."""
        check(lib().yk_render_guides_ids_device(self.h, scene.h, C.byref(camera.matrices), int(res[0]), int(res[1]), _vp(d_guides_ptr), _vp(d_ids_ptr), _vp(stream)), self.h)

    def render_guides_through_device(self, scene, camera, res, d_guides_ptr, d_ids_ptr, d_through_ptr, max_through=4, stream=None):
        """yk_render_guides_through_device: render_guides_ids_device following glass for up to max_through interfaces, with
        res[0] * res[1] uint32 (4-byte aligned) of interfaces crossed beside the records; any pointer may be None, not all
        three, no two buffers may overlap.  No read-back: ordered on `stream` like the other guide calls."""
        check(lib().yk_render_guides_through_device(self.h, scene.h, C.byref(camera.matrices), int(res[0]), int(res[1]), int(max_through), _vp(d_guides_ptr), _vp(d_ids_ptr), _vp(d_through_ptr), _vp(stream)), self.h)

    def surface_motion_device(self, scene, d_ids_ptr, d_guides_ptr, d_prev_points_ptr, res, d_out_ptr, stream=None, d_prev_spheres_ptr=None, d_prev_transforms_ptr=_AT_REST):
        """yk_surface_motion_device: device ids and guides of the current geometry and the PREVIOUS vertex array on the device
        (3 floats for each of the scene's vertices: the caller answers for its length) -> res[0] * res[1] device yk_motion
        records, enqueued on `stream` (default: the context's) without waiting; one launch, no allocation.  With
        d_prev_spheres_ptr (the scene's n_spheres yk_sphere_desc records from before the last edit, on the device)
        yk_surface_motion_spheres_device: spheres that moved carry their points along.  With d_prev_transforms_ptr (the
        scene's n_meshes yk_mesh_transform records of the previous Scene.transform on the device, 4-byte aligned; None or 0:
        the scene stood at rest) and d_prev_points_ptr None, yk_surface_motion_transforms_device: the previous vertices
        are made of the scene's rest pose."""
        if d_prev_transforms_ptr is not _AT_REST:
            if d_prev_points_ptr:
                raise ValueError("d_prev_points_ptr and d_prev_transforms_ptr are two ways to say where the vertices stood: give one")
            check(lib().yk_surface_motion_transforms_device(self.h, scene.h, _vp(d_ids_ptr), _vp(d_guides_ptr), _vp(d_prev_transforms_ptr), _vp(d_prev_spheres_ptr), int(res[0]), int(res[1]),
                                                            _vp(d_out_ptr), _vp(stream)), self.h)
            return
        if d_prev_spheres_ptr:
            check(lib().yk_surface_motion_spheres_device(self.h, scene.h, _vp(d_ids_ptr), _vp(d_guides_ptr), _vp(d_prev_points_ptr), _vp(d_prev_spheres_ptr), int(res[0]), int(res[1]), _vp(d_out_ptr),
                                                         _vp(stream)), self.h)
            return
        check(lib().yk_surface_motion_device(self.h, scene.h, _vp(d_ids_ptr), _vp(d_guides_ptr), _vp(d_prev_points_ptr), int(res[0]), int(res[1]), _vp(d_out_ptr), _vp(stream)), self.h)

    def surface_albedo_device(self, scene, d_ids_ptr, res, d_out_ptr, stream=None):
        """yk_surface_albedo_device: device ids -> res[0] * res[1] device yk_albedo records (both 16-byte aligned), enqueued
        on `stream` (default: the context's) without waiting."""
        check(lib().yk_surface_albedo_device(self.h, scene.h, _vp(d_ids_ptr), int(res[0]), int(res[1]), _vp(d_out_ptr), _vp(stream)), self.h)

    def albedo_mean_device(self, scene, d_ids_ss_ptr, res, s, d_out_ptr, stream=None):
        """yk_albedo_mean_device: the device ids of the (s * res[0]) x (s * res[1]) film -> res[0] * res[1] device yk_albedo
        records (both 16-byte aligned), enqueued on `stream` (default: the context's) without waiting; one launch, no
        allocation."""
        check(lib().yk_albedo_mean_device(self.h, scene.h, _vp(d_ids_ss_ptr), int(res[0]), int(res[1]), int(s), _vp(d_out_ptr), _vp(stream)), self.h)

    def render_albedo_mean_device(self, scene, camera_ss, res, s, d_out_ptr, stream=None):
        """yk_render_albedo_mean_device: the pixel-mean albedo of the film `res` into res[0] * res[1] device yk_albedo records
        (16-byte aligned), ordered on `stream` (default: the context's) without waiting on the host.  `camera_ss` is the
        Camera of the s-times larger film (Camera(params, supersampled(film_settings, s)))."""
        check(lib().yk_render_albedo_mean_device(self.h, scene.h, C.byref(camera_ss.matrices), int(res[0]), int(res[1]), int(s), _vp(d_out_ptr), _vp(stream)), self.h)

    def upsample_device(self, d_low_film_ptr, d_low_guides_ptr, low_res, d_guides_ptr, params, tile_dim, samples, d_out_ptr, stream=None, low_albedo=None, albedo=None, d_out_weight_ptr=None):
        """yk_upsample_device: the device film and guides of the low_res film and the device guides of the s-times larger one
        -> s * s * low_res[0] * low_res[1] device RGB pixels (and float weights where d_out_weight_ptr is given), enqueued on
        `stream` (default: the context's) without waiting; one launch.  low_albedo / albedo: the device pointers of
        albedo_mean_device's and surface_albedo_device's records, both or neither.  `samples` is the LOW film's host table
        (or None), copied before the call returns."""
        d = _upsample_desc(params)
        samples = _blend_samples(low_res, tile_dim, samples)
        check(lib().yk_upsample_device(self.h, C.byref(d), _vp(d_low_film_ptr), _vp(d_low_guides_ptr), _vp(low_albedo), int(low_res[0]), int(low_res[1]), int(tile_dim), _p(samples), _vp(d_guides_ptr),
                                       _vp(albedo), _vp(d_out_ptr), _vp(d_out_weight_ptr), _vp(stream)), self.h)

    def reproject_history_moved_device(self, d_prev_history_ptr, d_prev_guides_ptr, prev_camera, d_guides_ptr, d_motion_ptr, res, params, d_out_history_ptr, stream=None):
        """yk_history_reproject_moved_device: reproject_history_device through the device motion records of
        surface_motion_device (all 16-byte aligned), enqueued on `stream` (default: the context's) without waiting."""
        d = _temporal_desc(params)
        check(lib().yk_history_reproject_moved_device(self.h, C.byref(d), _vp(d_prev_history_ptr), _vp(d_prev_guides_ptr), C.byref(prev_camera.matrices), _vp(d_guides_ptr), _vp(d_motion_ptr), int(res[0]), int(res[1]), _vp(d_out_history_ptr), _vp(stream)), self.h)

    def blend_history_device(self, d_film_ptr, res, params, tile_dim, samples, d_history_ptr, d_out_history_ptr, d_out_rgb_ptr, stream=None):
        """yk_history_blend_device: device film + device history (or None) -> device history and / or device RGB (None = not
        wanted; they may be the inputs), enqueued on `stream` (default: the context's) without waiting; `samples` is a host
        table (or None), copied before the call returns."""
        d = _temporal_desc(params)
        samples = _blend_samples(res, tile_dim, samples)
        check(lib().yk_history_blend_device(self.h, C.byref(d), _vp(d_film_ptr), int(res[0]), int(res[1]), int(tile_dim), _p(samples), _vp(d_history_ptr), _vp(d_out_history_ptr), _vp(d_out_rgb_ptr), _vp(stream)), self.h)

    def blend_moments_device(self, d_film_ptr, res, params, tile_dim, samples, d_moments_ptr, d_out_moments_ptr, stream=None):
        """yk_moments_blend_device: device film + device moments (or None) -> device moments (may be the input), enqueued on
        `stream` (default: the context's) without waiting; `params` is blend_history_device's TemporalParams."""
        d = _temporal_desc(params)
        samples = _blend_samples(res, tile_dim, samples)
        check(lib().yk_moments_blend_device(self.h, C.byref(d), _vp(d_film_ptr), int(res[0]), int(res[1]), int(tile_dim), _p(samples), _vp(d_moments_ptr), _vp(d_out_moments_ptr), _vp(stream)), self.h)

    def rectify_history_device(self, d_film_ptr, res, params, tile_dim, samples, d_history_ptr, d_out_history_ptr, stream=None, moments=None, out_moments=None):
        """yk_history_rectify_device: device film + device history -> device history (may be the input), enqueued on
        `stream` (default: the context's) without waiting; one launch.  moments / out_moments: the device pointers of the
        moments beside the history and of their output (may be the same), both or neither.  `samples` is a host table (or
        None), copied before the call returns."""
        d = _rectify_desc(params)
        samples = _blend_samples(res, tile_dim, samples)
        check(lib().yk_history_rectify_device(self.h, C.byref(d), _vp(d_film_ptr), int(res[0]), int(res[1]), int(tile_dim), _p(samples), _vp(d_history_ptr), _vp(moments), _vp(d_out_history_ptr), _vp(out_moments), _vp(stream)), self.h)

    def despeckle_device(self, d_film_ptr, res, params, tile_dim, samples, d_out_ptr, stream=None, mask=None, counts=None):
        """yk_despeckle_device: device film -> device film (another buffer: the pass does not run in place), enqueued on
        `stream` (default: the context's) without waiting; one launch.  Each of the film, the output, mask (one byte a
        pixel) and counts (two uint32 words) is a torch tensor or a device address; mask and counts may be None.
        `samples` is a host table (or None), copied before the call returns."""
        d = _despeckle_desc(params)
        samples = _blend_samples(res, tile_dim, samples)
        ptr = [a.data_ptr() if hasattr(a, "data_ptr") else a for a in (d_film_ptr, d_out_ptr, mask, counts)]
        check(lib().yk_despeckle_device(self.h, C.byref(d), _vp(ptr[0]), int(res[0]), int(res[1]), int(tile_dim), _p(samples), _vp(ptr[1]), _vp(ptr[2]), _vp(ptr[3]), _vp(stream)), self.h)

    def variance_device(self, d_moments_ptr, d_film_ptr, d_guides_ptr, res, params, tile_dim, samples, d_out_ptr, stream=None, albedo=None):
        """yk_variance_device: device moments (or None), film, guides and albedo (or None) -> res[0] * res[1] device floats,
        enqueued on `stream` (default: the context's) without waiting; one launch."""
        d = _variance_desc(params)
        samples = _blend_samples(res, tile_dim, samples)
        check(lib().yk_variance_device(self.h, C.byref(d), _vp(d_moments_ptr), _vp(d_film_ptr), _vp(d_guides_ptr), _vp(albedo), int(res[0]), int(res[1]), int(tile_dim), _p(samples), _vp(d_out_ptr), _vp(stream)), self.h)

    def denoise_variance_device(self, d_film_ptr, d_guides_ptr, d_variance_ptr, res, params, tile_dim, samples, d_out_ptr, stream=None, albedo=None):
        """yk_denoise_variance_device: denoise_device with the device variance image of variance_device and a
        VarianceParams; d_out_ptr may be the film."""
        d = _variance_desc(params)
        samples = _blend_samples(res, tile_dim, samples)
        check(lib().yk_denoise_variance_device(self.h, C.byref(d), _vp(d_film_ptr), _vp(d_guides_ptr), _vp(d_variance_ptr), _vp(albedo), int(res[0]), int(res[1]), int(tile_dim), _p(samples), _vp(d_out_ptr), _vp(stream)), self.h)

    def adaptive_select_device(self, d_stats_ptr, res, params, pixel_list, stream=None):
        """yk_adaptive_select_device: device statistics -> `pixel_list` (a PixelList of the same resolution); returns the
        number selected.  Three launches on `stream` (default: the context's), then the count is read back: it waits."""
        d = _adaptive_desc(params)
        n = C.c_uint32(0)
        check(lib().yk_adaptive_select_device(self.h, C.byref(d), _vp(d_stats_ptr), int(res[0]), int(res[1]), pixel_list.h, C.byref(n), _vp(stream)), self.h)
        pixel_list.n = n.value
        return n.value

    def adaptive_accumulate_device(self, pixel_list, d_passes_ptr, n_passes, res, d_film_sum_ptr, d_stats_ptr, stream=None):
        """yk_adaptive_accumulate_device: the (n_passes, n, 3) device passes of `pixel_list` folded into the device film sums
        and statistics, one launch on `stream` (default: the context's) without waiting."""
        check(lib().yk_adaptive_accumulate_device(self.h, pixel_list.h, _vp(d_passes_ptr), int(n_passes), int(res[0]), int(res[1]), _vp(d_film_sum_ptr), _vp(d_stats_ptr), _vp(stream)), self.h)

    def adaptive_resolve_device(self, d_film_sum_ptr, d_stats_ptr, res, d_out_rgb_ptr, d_out_variance_ptr, stream=None):
        """yk_adaptive_resolve_device: device film sums and statistics -> the device mean film and / or the variance of the
        mean (None = not wanted), one launch on `stream` (default: the context's) without waiting."""
        check(lib().yk_adaptive_resolve_device(self.h, _vp(d_film_sum_ptr), _vp(d_stats_ptr), int(res[0]), int(res[1]), _vp(d_out_rgb_ptr), _vp(d_out_variance_ptr), _vp(stream)), self.h)

    @property
    def stream_handle(self):
        """The context's hipStream_t as an integer (yk_context_stream): wrap it, e.g. with
        torch.cuda.ExternalStream, to order other device work after a render."""
        return int(lib().yk_context_stream(self.h) or 0)

    def close(self):
        if getattr(self, "h", None):
            lib().yk_context_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _device_addresses(given, table, ctx, stream):
    """The device arrays of Scene.from_device and Scene.update: `given` maps names to torch tensors, raw device addresses
    (int) or None, `table` maps every name to (accepted element types, expected element count).  Checks every tensor's
    element type, contiguity and element count first and only then where the tensors are (ValueError); an address is
    taken as it is.  Returns ({name: address or None}, the stream to pass on: an int or None).  With `stream` None the
    current torch stream of the first tensor's device is waited for."""
    address, tensors = {}, []
    for name, (dtypes, expected) in table.items():
        a = given.get(name)
        if a is None or isinstance(a, (int, np.integer)):
            address[name] = int(a) if a else None
            continue
        if not hasattr(a, "data_ptr"):
            raise ValueError(f"{name}: expected a torch tensor or a device address, got {type(a).__name__}")
        if str(a.dtype).replace("torch.", "") not in dtypes:
            raise ValueError(f"{name}: element type {a.dtype}, expected {' or '.join(dtypes)}")
        if not a.is_contiguous():
            raise ValueError(f"{name}: the tensor is not contiguous")
        if a.numel() != expected:
            raise ValueError(f"{name}: {a.numel()} elements, expected {expected}")
        tensors.append((name, a))
    for name, a in tensors:  # ... and only then where they are
        if not a.is_cuda or a.device.index != ctx.device:
            raise ValueError(f"{name}: the tensor is on {a.device}, not on the context's device {ctx.device}")
        address[name] = a.data_ptr() or None
    if stream is None and tensors:
        import torch

        torch.cuda.current_stream(tensors[0][1].device).synchronize()
    elif stream is not None and not isinstance(stream, int):
        stream = stream.cuda_stream
    return address, stream


class Scene:
    """scene/mod.rs:41-49: shapes + BVH + lights + background.  `ctx=None` builds
    the BVH on the host only (no GPU needed)."""

    def __init__(self, ctx, scene_data):
        self.ctx = ctx
        self.data = scene_data
        d, self._keep = scene_data.desc(LightFactory)
        self.n_lights = int(d.n_lights)
        h = C.c_void_p()
        check(lib().yk_scene_create(ctx.h if ctx else None, C.byref(d), C.byref(h)), ctx.h if ctx else None)
        self.h = h
        self._keep = None  # the library copied everything it needs

    # name -> (pointer type of the yk_scene_desc field, accepted element types, elements per vertex "v" | triangle "t" | shape "s")
    DEVICE_ARRAYS = {
        "points": (abi.f32p, ("float32",), "v", 3),
        "normals": (abi.f32p, ("float32",), "v", 3),
        "uvs": (abi.f32p, ("float32",), "v", 2),
        "indices": (abi.u32p, ("uint32", "int32"), "t", 3),
        "tri_mesh": (abi.u32p, ("uint32", "int32"), "t", 1),
        "tri_material": (abi.i32p, ("int32",), "t", 1),
        "tri_area_light": (abi.i32p, ("int32",), "t", 1),
        "shape_order": (abi.u32p, ("uint32", "int32"), "s", 1),
    }

    @classmethod
    def from_device(cls, ctx, scene_data, arrays, stream=None):
        """yk_scene_create_device: the scene of `scene_data` from geometry that is in device memory already.

        `arrays` maps the names of Scene.DEVICE_ARRAYS to torch tensors on the context's device or to raw device addresses
        (int); a name left out (or None) is a NULL array, as in yk_scene_desc.  A tensor's element type, contiguity,
        element count and device are checked here (ValueError) before anything reaches the library; an address is taken
        as it is.  `scene_data` supplies the small tables (meshes, spheres, materials, lights, textures), the BVH settings
        and the counts: its own large arrays are read for their shapes only.  `stream`: the hipStream_t (an int, or a
        torch stream) on which the arrays were produced; None waits for the current torch stream of a tensor's device
        instead.  The call is synchronous and the scene keeps copies: the tensors may be freed or overwritten after it."""
        unknown = set(arrays) - set(cls.DEVICE_ARRAYS)
        if unknown:
            raise ValueError(f"unknown device arrays {sorted(unknown)}; the names are {sorted(cls.DEVICE_ARRAYS)}")
        counts = {"v": int(scene_data.points.shape[0]), "t": int(scene_data.indices.shape[0])}
        counts["s"] = counts["t"] + len(scene_data.spheres)
        address, stream = _device_addresses(arrays, {name: (dtypes, k * counts[per]) for name, (_, dtypes, per, k) in cls.DEVICE_ARRAYS.items()}, ctx, stream)
        self = cls.__new__(cls)
        self.ctx, self.data = ctx, scene_data
        d, keep = scene_data.desc(LightFactory)
        for name, (ptype, _, _, _) in cls.DEVICE_ARRAYS.items():
            setattr(d, name, C.cast(C.c_void_p(address[name]), ptype))
        self.n_lights = int(d.n_lights)
        h = C.c_void_p()
        check(lib().yk_scene_create_device(ctx.h, C.byref(d), _vp(stream), C.byref(h)), ctx.h)
        self.h = h
        del keep
        return self

    def close(self):
        if getattr(self, "h", None):
            lib().yk_scene_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        i = SceneInfo()
        check(lib().yk_scene_get_info(self.h, C.byref(i)))
        return i

    def build_info(self):
        """yk_scene_get_build_info: who built the tree (_ffi.BVH_BUILDER_NAMES), why not the device (_ffi.BVH_REASON_NAMES), phase seconds."""
        i = BvhBuildInfo()
        check(lib().yk_scene_get_build_info(self.h, C.byref(i)))
        return i

    def layout_info(self):
        """yk_scene_get_layout_info: who laid the traversal records out (abi.LAYOUT_*), why not the device (abi.LAYOUT_REASON_*),
        whether the host copy of the tree exists yet, and the root ref / tree-top sizes / wide flags the kernels are handed."""
        i = abi.SceneLayoutInfo()
        check(lib().yk_scene_get_layout_info(self.h, C.byref(i)))
        return i

    def update(self, points, normals=None, stream=None):
        """yk_scene_update / yk_scene_update_device: the scene's vertices move, its tree is refitted in place (topology and
        leaf order kept) and its records are rewritten.  `points` is (n_vertices, 3) float32 for the scene's own vertex
        count, `normals` the same or None to keep the scene's normals.  numpy arrays go to yk_scene_update (which follows
        the scene's layout); torch tensors on the context's device, or raw device addresses (int), go to
        yk_scene_update_device, which always takes the device route — `stream` as in from_device.  A tensor's element
        type, contiguity, element count and device are checked here (ValueError) before the library is reached; an
        address is taken as it is.  Every coordinate must be finite.  With numpy input `self.data` becomes a copy that
        carries the new arrays; with tensors or addresses it is left alone and keeps describing the geometry the scene
        was created from."""
        nv = int(self.data.points.shape[0])
        given = {"points": points, "normals": normals}
        if all(a is None or isinstance(a, np.ndarray) or isinstance(a, (list, tuple)) for a in given.values()):
            host = {}
            for name, a in given.items():
                if a is None:
                    host[name] = None
                    continue
                a = np.ascontiguousarray(a, dtype=np.float32)
                if a.size != 3 * nv:
                    raise ValueError(f"{name}: {a.size} elements, expected {3 * nv}")
                host[name] = a.reshape(nv, 3)
            ctx_h = self.ctx.h if self.ctx else None
            check(lib().yk_scene_update(ctx_h, self.h, _p(host["points"]), _p(host["normals"])), ctx_h)
            import copy

            self.data = copy.copy(self.data)
            if host["points"] is not None:
                self.data.points = host["points"]
            if host["normals"] is not None:
                self.data.normals = host["normals"]
            return
        if self.ctx is None:
            raise ValueError("a host-only scene is updated with numpy arrays")
        address, stream = _device_addresses(given, {name: (("float32",), 3 * nv) for name in given}, self.ctx, stream)
        check(lib().yk_scene_update_device(self.ctx.h, self.h, _vp(address["points"]), _vp(address["normals"]), _vp(stream)), self.ctx.h)

    def update_info(self):
        """yk_scene_get_update_info: how many updates ran, the last one's route (abi.UPDATE_ROUTE_*) and reason
        (abi.LAYOUT_REASON_*), the level launches and device bytes of the plan, and the last update's phase seconds."""
        i = abi.SceneUpdateInfo()
        check(lib().yk_scene_get_update_info(self.h, C.byref(i)))
        return i

    def edit(self, spheres=None, lights=None, materials=None, background=None, stream=None):
        """yk_scene_apply_edit / yk_scene_apply_edit_device: the scene's spheres, lights, materials and background change
        in place; its triangles stay.  Every table is None (keep) or as long as the scene's own: `spheres`, `lights` and
        `materials` are lists of what SceneData holds for them (lights may also be ready abi.LightDesc values), `background`
        is three floats.  Counts and light kinds cannot change; a material's kind and a sphere's material can.  `spheres`
        may also be a torch tensor on the context's device, or a raw device address (int), of n_spheres *
        sizeof(yk_sphere_desc) bytes (abi.SPHERE_DTYPE records; a tensor is uint8 with that many elements, or int32 / float32
        with a quarter of them): it goes to yk_scene_apply_edit_device, which takes the device route — `stream` as in
        from_device.  A tensor's element type, contiguity, element count and device are checked here (ValueError) before the
        library is reached.  With host input `self.data` becomes a copy that carries the new tables; a sphere table in
        device memory leaves its spheres as they were."""
        import copy

        new = copy.copy(self.data)
        e, keep = abi.SceneEdit(), []
        d_spheres = None
        n_spheres = len(self.data.spheres)
        if spheres is not None and (hasattr(spheres, "data_ptr") or isinstance(spheres, (int, np.integer))):
            if self.ctx is None:
                raise ValueError("a host-only scene is edited with host tables")
            n_bytes = n_spheres * abi.SPHERE_DTYPE.itemsize
            per = spheres.element_size() if hasattr(spheres, "element_size") else 1
            address, stream = _device_addresses({"spheres": spheres}, {"spheres": (("uint8",) if per == 1 else ("int32", "float32"), n_bytes // per)}, self.ctx, stream)
            d_spheres = address["spheres"]
        elif spheres is not None:
            if len(spheres) != n_spheres:
                raise ValueError(f"spheres: {len(spheres)} records, the scene has {n_spheres}")
            new.spheres = list(spheres)
            keep.append(new.sphere_descs())
            e.spheres = C.cast(keep[-1], C.POINTER(abi.SphereDesc))
        if lights is not None:
            n_lights = len(self.data.lights) if self.data.light_structs is None else len(self.data.light_structs)
            if len(lights) != n_lights:
                raise ValueError(f"lights: {len(lights)} records, the scene has {n_lights}")
            if lights and isinstance(lights[0], abi.LightDesc):
                new.light_structs = list(lights)
            else:
                new.lights, new.light_structs = list(lights), None
            keep.append(new.light_descs(LightFactory))
            e.lights = C.cast(keep[-1], C.POINTER(abi.LightDesc))
        if materials is not None:
            if len(materials) != len(self.data.materials):
                raise ValueError(f"materials: {len(materials)} records, the scene has {len(self.data.materials)}")
            new.materials = list(materials)
            keep.append(new.material_descs())
            e.materials = C.cast(keep[-1], C.POINTER(abi.MaterialDesc))
        if background is not None:
            if len(background) != 3:
                raise ValueError("background is three floats")
            new.background = tuple(float(x) for x in background)
            keep.append(abi.f3(new.background))
            e.background = C.cast(keep[-1], abi.f32p)
        ctx_h = self.ctx.h if self.ctx else None
        if d_spheres is not None:
            check(lib().yk_scene_apply_edit_device(ctx_h, self.h, C.byref(e), _vp(d_spheres), _vp(stream)), ctx_h)
        else:
            check(lib().yk_scene_apply_edit(ctx_h, self.h, C.byref(e)), ctx_h)
        self.data = new

    def edit_info(self):
        """yk_scene_get_edit_info: how many edits ran, the last one's route (abi.UPDATE_ROUTE_*) and reason
        (abi.LAYOUT_REASON_*), what it rewrote (abi.EDIT_* bits) and its phase seconds."""
        i = abi.SceneEditInfo()
        check(lib().yk_scene_get_edit_info(self.h, C.byref(i)))
        return i

    def transform(self, transforms, stream=None):
        """yk_scene_transform / yk_scene_transform_device: every mesh of the scene is placed by a matrix, relative to its
        rest pose (the points and normals after creation or the last update); absolute, not cumulative.  Host input —
        an (n_meshes, 4, 4) array, a list of n_meshes matrices with None for the identity (both through
        abi.pack_mesh_transforms, which inverts in float64), or (n_meshes,) abi.MESH_TRANSFORM_DTYPE records whose pairs
        are the caller's — goes to yk_scene_transform, which follows the scene's layout.  A torch tensor on the context's
        device, or a raw device address (int), holding the packed records (uint8 with 128 * n_meshes elements, or int32 /
        float32 with a quarter of them) goes to yk_scene_transform_device, which takes the device route — `stream` and
        the argument checks (ValueError) as in Scene.update.  `self.data` keeps describing the rest pose."""
        n_meshes = len(self.data.meshes)
        if hasattr(transforms, "data_ptr") or isinstance(transforms, (int, np.integer)):
            if self.ctx is None:
                raise ValueError("a host-only scene is transformed with host records")
            n_bytes = n_meshes * abi.MESH_TRANSFORM_DTYPE.itemsize
            per = transforms.element_size() if hasattr(transforms, "element_size") else 1
            address, stream = _device_addresses({"transforms": transforms}, {"transforms": (("uint8",) if per == 1 else ("int32", "float32"), n_bytes // per)}, self.ctx, stream)
            check(lib().yk_scene_transform_device(self.ctx.h, self.h, _vp(address["transforms"]), _vp(stream)), self.ctx.h)
            return
        if transforms is not None:
            if not (isinstance(transforms, np.ndarray) and transforms.dtype == abi.MESH_TRANSFORM_DTYPE):
                transforms = abi.pack_mesh_transforms(transforms)
            if transforms.shape != (n_meshes,):
                raise ValueError(f"transforms: {transforms.shape} records, the scene has {n_meshes} meshes")
            transforms = np.ascontiguousarray(transforms)
        ctx_h = self.ctx.h if self.ctx else None
        check(lib().yk_scene_transform(ctx_h, self.h, _p(transforms)), ctx_h)

    def transform_info(self):
        """yk_scene_get_transform_info: how many transforms ran, the last one's route and reason, its moved and flipped
        meshes, the bytes kept of the rest pose, tree_cost and tree_cost_rest, and the phase seconds."""
        i = abi.SceneTransformInfo()
        check(lib().yk_scene_get_transform_info(self.h, C.byref(i)))
        return i

    def device_records(self, which):
        """yk_scene_read_records: one of the scene's device record buffers (abi.RECORDS_* or a name of abi.RECORD_NAMES) as uint8."""
        if isinstance(which, str):
            which = abi.RECORD_NAMES.index(which)
        n = C.c_size_t(0)
        check(lib().yk_scene_read_records(self.h, int(which), None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint8)
        check(lib().yk_scene_read_records(self.h, int(which), _p(out), out.nbytes, C.byref(n)))
        return out

    def export_bvh(self):
        i = self.info()
        nodes = np.zeros(i.n_nodes, dtype=abi.BVH_NODE_DTYPE)
        order = np.zeros(i.n_shapes, dtype=np.uint32)
        check(lib().yk_scene_export_bvh(self.h, _p(nodes), _p(order)))
        return nodes, order

    def node_bounds(self, level):
        """BoundingVolumeHierarchy::node_bounds (bvh.rs:121-157): (n, 2, 3) float32 (p_min, p_max); level -1 = every
        node's box, 0 = the root's."""
        n = lib().yk_scene_node_bounds(self.h, int(level), None, 0)
        out = np.zeros((n, 2, 3), dtype=np.float32)
        lib().yk_scene_node_bounds(self.h, int(level), _p(out), n)
        return out

    # per-stage entry points ---------------------------------------------------
    def intersect(self, o, d, t_max=None, counters=False):
        """BoundingVolumeHierarchy::intersect for n rays (bvh.rs:160-232)."""
        o = np.ascontiguousarray(o, dtype=np.float32)
        d = np.ascontiguousarray(d, dtype=np.float32)
        n = o.shape[0]
        tm = None if t_max is None else np.ascontiguousarray(t_max, dtype=np.float32)
        r = dict(shape=np.zeros(n, dtype=np.int32), t=np.zeros(n, dtype=np.float32), bary=np.zeros((n, 3), dtype=np.float32))
        if counters:
            r.update(node_tests=np.zeros(n, dtype=np.uint32), node_hits=np.zeros(n, dtype=np.uint32), shape_tests=np.zeros(n, dtype=np.uint32))
        check(
            lib().yk_trace_closest(self.ctx.h, self.h, n, _p(o), _p(d), _p(tm), _p(r["shape"]), _p(r["t"]), _p(r["bary"]), _p(r.get("node_tests")), _p(r.get("node_hits")), _p(r.get("shape_tests"))),
            self.ctx.h,
        )
        return r

    def any_intersect(self, o, d, t_max, area_light=None):
        """BoundingVolumeHierarchy::any_intersect (bvh.rs:235-302)."""
        o = np.ascontiguousarray(o, dtype=np.float32)
        d = np.ascontiguousarray(d, dtype=np.float32)
        tm = np.ascontiguousarray(t_max, dtype=np.float32)
        al = None if area_light is None else np.ascontiguousarray(area_light, dtype=np.int32)
        out = np.zeros(o.shape[0], dtype=np.uint8)
        check(lib().yk_trace_any(self.ctx.h, self.h, o.shape[0], _p(o), _p(d), _p(tm), _p(al), _p(out)), self.ctx.h)
        return out


def refit_bvh(nodes, order, shape_bounds):
    """yk_bvh_refit: the refit rule on the host over an exported tree.  nodes: abi.BVH_NODE_DTYPE, order: the leaf order
    (both as Scene.export_bvh returns them), shape_bounds: (n_shapes, 6) or (n_shapes, 2, 3) float32, min.xyz and max.xyz per
    SOURCE shape.  -> a refitted copy of `nodes`; links, axes, counts and flags are untouched."""
    out = np.array(nodes, dtype=abi.BVH_NODE_DTYPE).copy()
    order = np.ascontiguousarray(order, dtype=np.uint32)
    sb = np.ascontiguousarray(shape_bounds, dtype=np.float32).reshape(-1, 6)
    check(lib().yk_bvh_refit(_p(out), len(out), _p(order), len(sb), _p(sb)))
    return out


# --------------------------------------------------------------------------- several GPUs
def _mcheck(status, m):
    if status != _ffi.YK_OK:
        buf = C.create_string_buffer(512)
        lib().yk_multi_last_error(m, buf, 512)
        raise YukiError(status, buf.value.decode(errors="replace") or lib().yk_status_string(status).decode())


class Multi:
    """The GPUs of one process (yk_multi): a context and a host thread per device; tiles of the
    film's spiral are dealt round-robin (render_manager.rs:206-210), the slabs meet on devices[0]
    through RCCL and Film::update_tile runs there."""

    SHARED_DEVICES, PEER_COPY = 1, 2  # yk_multi_create_ex flags

    def __init__(self, devices, flags=0, **options):
        """flags: Multi.SHARED_DEVICES — ranks may name the same device (G ranks on one GPU: what a one-GPU box can run of
        the G > 1 path; the slabs travel by device copies); Multi.PEER_COPY — hipMemcpyPeerAsync instead of RCCL."""
        devices = [int(d) for d in devices]
        arr = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        check(lib().yk_multi_create_ex(arr, len(devices), int(flags), C.byref(h)) if flags else lib().yk_multi_create(arr, len(devices), C.byref(h)))
        self.h = h
        self.devices = devices
        for k, v in options.items():
            self.set_option(k, v)

    def set_option(self, key, value):
        _mcheck(lib().yk_multi_set_option(self.h, key.encode(), int(value)), self.h)

    def scene(self, scene_data):
        return MultiScene(self, scene_data)

    def film(self, settings):
        return MultiFilm(self, settings)

    def render_film(self, scene, camera, sampler, integrator, film, want_host=True, want_stats=True, cancel=None):
        """Integrator::render for every tile of the film on its device, exchange, Film::update_tile.
        Returns (film (h, w, 3) float32 or None, RenderStats or None)."""
        out = np.zeros((film.res[1], film.res[0], 3), dtype=np.float32) if want_host else None
        stats = RenderStats() if want_stats else None
        cb = _ffi.CANCEL_FN(lambda _u: 1 if cancel() else 0) if cancel else None
        _mcheck(
            lib().yk_multi_render_film(self.h, scene.h, C.byref(camera.matrices), C.byref(sampler), C.byref(integrator), film.h, _p(out), C.byref(stats) if want_stats else None, C.cast(cb, C.c_void_p) if cb else None, None),
            self.h,
        )
        return out, stats

    def accumulate_film(self, scene, camera, sampler, integrator, film, first_sample, n_passes=1, want_host=True, want_stats=True, cancel=None):
        """The accumulating film over all devices (yk_multi_accumulate_film): passes first_sample .. + n_passes - 1 of every
        tile, each added to the film on device 0 (film.rs:260-272).  clear_film() starts a new accumulation."""
        out = np.zeros((film.res[1], film.res[0], 3), dtype=np.float32) if want_host else None
        stats = RenderStats() if want_stats else None
        cb = _ffi.CANCEL_FN(lambda _u: 1 if cancel() else 0) if cancel else None
        _mcheck(
            lib().yk_multi_accumulate_film(self.h, scene.h, C.byref(camera.matrices), C.byref(sampler), C.byref(integrator), film.h, int(first_sample), int(n_passes), _p(out), C.byref(stats) if want_stats else None, C.cast(cb, C.c_void_p) if cb else None, None),
            self.h,
        )
        return out, stats

    def clear_film(self, film):
        _mcheck(lib().yk_multi_film_clear(self.h, film.h), self.h)

    def interrupt(self):
        """yk_multi_interrupt: stop the frame in flight on every rank (any thread)."""
        check(lib().yk_multi_interrupt(self.h))

    def sync(self):
        _mcheck(lib().yk_multi_sync(self.h), self.h)

    def close(self):
        if getattr(self, "h", None):
            lib().yk_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiScene:
    def __init__(self, multi, scene_data):
        self.multi = multi
        d, keep = scene_data.desc(LightFactory)
        h = C.c_void_p()
        _mcheck(lib().yk_multi_scene_create(multi.h, C.byref(d), C.byref(h)), multi.h)
        self.h = h

    def info(self):
        i = SceneInfo()
        check(lib().yk_multi_scene_get_info(self.h, C.byref(i)))
        return i

    def close(self):
        if getattr(self, "h", None):
            lib().yk_multi_scene_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiFilm:
    def __init__(self, multi, settings):
        self.multi = multi
        self.res = tuple(settings.res)
        h = C.c_void_p()
        _mcheck(lib().yk_multi_film_create(multi.h, settings.res[0], settings.res[1], settings.tile_dim, C.byref(h)), multi.h)
        self.h = h

    @property
    def device_ptr(self):
        return int(lib().yk_multi_film_device_ptr(self.h) or 0)

    def close(self):
        if getattr(self, "h", None):
            lib().yk_multi_film_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Dist:
    """One process per GPU (yk_dist): join an RCCL communicator with this rank's context; gather()
    moves every rank's slab into rank 0's buffer on the context's stream."""

    ID_BYTES = 128  # YK_DIST_ID_BYTES

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * 128)()
        check(lib().yk_dist_unique_id(buf))
        return bytes(buf)

    def __init__(self, ctx, unique_id, rank, world):
        self.ctx = ctx
        idb = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        h = C.c_void_p()
        check(lib().yk_dist_create(ctx.h, idb, rank, world, C.byref(h)), ctx.h)
        self.h, self.rank, self.world = h, rank, world

    def gather(self, d_send_ptr, d_recv_ptr, count_floats, stream=None):
        check(lib().yk_dist_gather(self.h, C.c_void_p(d_send_ptr), _vp(d_recv_ptr), count_floats, _vp(stream)), self.ctx.h)

    def close(self):
        if getattr(self, "h", None):
            lib().yk_dist_destroy(self.h)
            self.h = None


# --------------------------------------------------------------------------- many workers, one device
class Combiner:
    """yk_combiner: Integrator::render called per tile from many worker threads (render_manager.rs:78-97), merged into shared
    submissions on `contexts` (one lane each).  `render` is what a worker thread calls; it blocks until its tile is done."""

    def __init__(self, contexts, max_tiles=0, linger_us=100):
        self.contexts = list(contexts)
        arr = (C.c_void_p * len(self.contexts))(*[c.h for c in self.contexts])
        h = C.c_void_p()
        check(lib().yk_combiner_create(arr, len(self.contexts), max_tiles, linger_us, C.byref(h)))
        self.h = h

    def _error(self, status):
        buf = C.create_string_buffer(512)
        lib().yk_combiner_last_error(self.h, buf, 512)
        return YukiError(status, buf.value.decode(errors="replace"))

    def render(self, integrator, scene, camera, sampler, tile, accumulating=False, cancel=None):
        """(tile_pixels[h*w,3], RenderStats) — integrators/mod.rs:120-185 for one FilmTile."""
        t = tile.as_struct() if isinstance(tile, FilmTile) else abi.Tile(*[int(v) for v in tile])
        w, h = t.x1 - t.x0, t.y1 - t.y0
        px = np.zeros((max(w, 0) * max(h, 0), 3), dtype=np.float32)
        stats = RenderStats()
        desc = integrator.desc if isinstance(integrator, Integrator) else integrator
        sample = (tile.sample if isinstance(tile, FilmTile) else 0) if accumulating else -1
        cb = _ffi.CANCEL_FN(lambda _u: 1 if cancel() else 0) if cancel else None
        st = lib().yk_combiner_render_tile(self.h, scene.h, C.byref(camera.matrices), C.byref(sampler), C.byref(desc), C.byref(t), sample, _p(px), C.byref(stats),
                                           C.cast(cb, C.c_void_p) if cb else None, None)
        if st != 0:
            raise self._error(st)
        return px, stats

    def info(self):
        out = _ffi.CombinerInfo()
        check(lib().yk_combiner_get_info(self.h, C.byref(out)))
        return out

    def close(self):
        if getattr(self, "h", None):
            lib().yk_combiner_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# --------------------------------------------------------------------------- integrators
class RayType:
    """integrators/mod.rs:83-90: the type of an IntegratorRay (yk_ray_type)."""

    Direct, Reflection, Refraction, Normal, Shadow = abi.RAY_DIRECT, abi.RAY_REFLECTION, abi.RAY_REFRACTION, abi.RAY_NORMAL, abi.RAY_SHADOW


class Integrator:
    """trait Integrator (integrators/mod.rs:92-186) over the HIP wavefront."""

    def __init__(self, ctx, desc):
        self.ctx = ctx
        self.desc = desc

    def render(self, scene, camera, sampler, tile, accumulating=False):
        """One tile; returns (tile_pixels[h*w,3], ray_count) — integrators/mod.rs:120-185."""
        t = tile.as_struct() if isinstance(tile, FilmTile) else abi.Tile(*[int(v) for v in tile])
        w, h = t.x1 - t.x0, t.y1 - t.y0
        if w <= 0 or h <= 0:
            raise YukiError(1, "Bounds2 with a dimension <= 0")
        if accumulating:  # one sample with global index tile.sample, raw value (integrators/mod.rs:146-161)
            sample = tile.sample if isinstance(tile, FilmTile) else 0
            tiles = np.array([(t.x0, t.y0, t.x1, t.y1)], dtype=abi.TILE_DTYPE)
            px, stats = self.render_tiles_accumulating(scene, camera, sampler, tiles, [sample])
            return px, stats.rays
        px = np.zeros((w * h, 3), dtype=np.float32)
        rays = C.c_uint64(0)
        check(lib().yk_render_tile(self.ctx.h, scene.h, C.byref(camera.matrices), C.byref(sampler), C.byref(self.desc), C.byref(t), _p(px), C.byref(rays)), self.ctx.h)
        return px, rays.value

    def render_tiles(self, scene, camera, sampler, tiles, cancel=None):
        """All tiles of one call as a single batch — the GPU-worker entry point.
        Returns (rgb tile-major [n_pixels,3], RenderStats)."""
        tiles = np.ascontiguousarray(tiles, dtype=abi.TILE_DTYPE)
        npx = int(((tiles["x1"].astype(np.int64) - tiles["x0"]) * (tiles["y1"].astype(np.int64) - tiles["y0"])).sum())
        out = np.zeros((npx, 3), dtype=np.float32)
        stats = RenderStats()
        cb = _ffi.CANCEL_FN(lambda _u: 1 if cancel() else 0) if cancel else None
        check(
            lib().yk_render_tiles(self.ctx.h, scene.h, C.byref(camera.matrices), C.byref(sampler), C.byref(self.desc), _p(tiles), len(tiles), _p(out), C.byref(stats), C.cast(cb, C.c_void_p) if cb else None, None),
            self.ctx.h,
        )
        return out, stats

    def render_tiles_accumulating(self, scene, camera, sampler, tiles, tile_samples, cancel=None, n_passes=1):
        """Integrator::render(accumulating=true) (integrators/mod.rs:146-161) for a list of
        (tile, FilmTile.sample) pairs: one sample per pixel, raw value.  Returns (rgb, stats);
        n_passes > 1 renders passes sample .. sample + n_passes - 1 at once: rgb is (n_passes, pixels, 3)."""
        tiles = np.ascontiguousarray(tiles, dtype=abi.TILE_DTYPE)
        ts = np.ascontiguousarray(tile_samples, dtype=np.uint16)
        if len(ts) != len(tiles):
            raise ValueError("one sample index per tile")
        npx = int(((tiles["x1"].astype(np.int64) - tiles["x0"]) * (tiles["y1"].astype(np.int64) - tiles["y0"])).sum())
        stats = RenderStats()
        cb = _ffi.CANCEL_FN(lambda _u: 1 if cancel() else 0) if cancel else None
        if n_passes != 1:
            out = np.zeros((n_passes, npx, 3), dtype=np.float32)
            check(
                lib().yk_render_tiles_accumulating_passes(self.ctx.h, scene.h, C.byref(camera.matrices), C.byref(sampler), C.byref(self.desc), _p(tiles), _p(ts), len(tiles), n_passes, _p(out), C.byref(stats), C.cast(cb, C.c_void_p) if cb else None, None),
                self.ctx.h,
            )
            return out, stats
        out = np.zeros((npx, 3), dtype=np.float32)
        check(
            lib().yk_render_tiles_accumulating(self.ctx.h, scene.h, C.byref(camera.matrices), C.byref(sampler), C.byref(self.desc), _p(tiles), _p(ts), len(tiles), _p(out), C.byref(stats), C.cast(cb, C.c_void_p) if cb else None, None),
            self.ctx.h,
        )
        return out, stats

    def render_tiles_device(self, scene, camera, sampler, tiles, d_out_ptr, stream=None, want_stats=True):
        """Radiance stays in HBM at `d_out_ptr` (e.g. a torch tensor's data_ptr())."""
        tiles = np.ascontiguousarray(tiles, dtype=abi.TILE_DTYPE)
        stats = RenderStats()
        check(
            lib().yk_render_tiles_device(self.ctx.h, scene.h, C.byref(camera.matrices), C.byref(sampler), C.byref(self.desc), _p(tiles), len(tiles), C.c_void_p(d_out_ptr), _vp(stream), C.byref(stats) if want_stats else None, None, None),
            self.ctx.h,
        )
        return stats

    def render_tile_list_samples_device(self, scene, camera, sampler, tile_list, first_sample, n_passes, d_out_ptr, stream=None, want_stats=False, cancel=None):
        """Passes first_sample .. first_sample + n_passes - 1 of every tile of a PLAIN tile list (the worker's accumulate loop,
        render_manager.rs:125-143), pass-major into HBM at `d_out_ptr`."""
        stats = RenderStats()
        cb = _ffi.CANCEL_FN(lambda _u: 1 if cancel() else 0) if cancel else None
        check(
            lib().yk_render_tile_list_samples_device(self.ctx.h, scene.h, C.byref(camera.matrices), C.byref(sampler), C.byref(self.desc), tile_list.h, int(first_sample), int(n_passes), C.c_void_p(d_out_ptr), _vp(stream), C.byref(stats) if want_stats else None, C.cast(cb, C.c_void_p) if cb else None, None),
            self.ctx.h,
        )
        return stats if want_stats else None

    def render_tile_list_device(self, scene, camera, sampler, tile_list, d_out_ptr, stream=None, want_stats=False, n_passes=1):
        """Render a prepared TileList into HBM at `d_out_ptr`; with want_stats=False the call only
        enqueues work on `stream` (no host synchronisation).  n_passes > 1 (accumulating list):
        that many passes at once, pass-major in `d_out_ptr`."""
        stats = RenderStats()
        if n_passes != 1:
            check(
                lib().yk_render_tile_list_passes_device(self.ctx.h, scene.h, C.byref(camera.matrices), C.byref(sampler), C.byref(self.desc), tile_list.h, n_passes, C.c_void_p(d_out_ptr), _vp(stream), C.byref(stats) if want_stats else None, None, None),
                self.ctx.h,
            )
            return stats if want_stats else None
        check(
            lib().yk_render_tile_list_device(self.ctx.h, scene.h, C.byref(camera.matrices), C.byref(sampler), C.byref(self.desc), tile_list.h, C.c_void_p(d_out_ptr), _vp(stream), C.byref(stats) if want_stats else None, None, None),
            self.ctx.h,
        )
        return stats if want_stats else None

    def render_pixel_list_device(self, scene, camera, sampler, pixel_list, n_passes, d_out_ptr, stream=None, want_stats=False, cancel=None):
        """yk_render_pixel_list_device: passes sample .. sample + n_passes - 1 of every entry of a PixelList, raw values,
        (n_passes, n, 3) pass-major into HBM at `d_out_ptr`: what the accumulating render writes for that pixel at that
        sample index."""
        stats = RenderStats()
        cb = _ffi.CANCEL_FN(lambda _u: 1 if cancel() else 0) if cancel else None
        check(
            lib().yk_render_pixel_list_device(self.ctx.h, scene.h, C.byref(camera.matrices), C.byref(sampler), C.byref(self.desc), pixel_list.h, int(n_passes), _vp(d_out_ptr), _vp(stream), C.byref(stats) if want_stats else None, C.cast(cb, C.c_void_p) if cb else None, None),
            self.ctx.h,
        )
        return stats if want_stats else None

    def render_adaptive(self, scene, camera, sampler, film_settings, params, film_sum=None, stats=None, stream=None, cancel=None):
        """yk_render_adaptive_device: rounds of select -> render -> fold on the device until nothing is selected (or
        params.max_rounds).  film_sum ((h, w, 3) float32) and stats ((h, w, 4) int32: the yk_pixel_stats records) are torch
        tensors on the context's device or device addresses; None makes cleared torch tensors.  It continues from what they
        hold: call again with a larger max_samples to refine.  Returns (film_sum, stats, abi.AdaptiveInfo)."""
        w, h = int(film_settings.res[0]), int(film_settings.res[1])
        if film_sum is None or stats is None:
            import torch

            dev = torch.device("cuda", self.ctx.device)
            film_sum = torch.zeros((h, w, 3), dtype=torch.float32, device=dev) if film_sum is None else film_sum
            stats = torch.zeros((h, w, 4), dtype=torch.int32, device=dev) if stats is None else stats
        address, stream = _device_addresses({"film_sum": film_sum, "stats": stats}, {"film_sum": (("float32",), w * h * 3), "stats": (("int32",), w * h * 4)}, self.ctx, stream)
        d = _adaptive_desc(params)
        info = abi.AdaptiveInfo()
        cb = _ffi.CANCEL_FN(lambda _u: 1 if cancel() else 0) if cancel else None
        check(
            lib().yk_render_adaptive_device(self.ctx.h, scene.h, C.byref(camera.matrices), C.byref(sampler), C.byref(self.desc), C.byref(d), w, h, _vp(address["film_sum"]), _vp(address["stats"]), _vp(stream), C.byref(info), C.cast(cb, C.c_void_p) if cb else None, None),
            self.ctx.h,
        )
        return film_sum, stats, info

    def li(self, scene, sampler, ray_o, ray_d, pixel_xy, sample_index, dimension=2, ray_counts=False):
        """Integrator::li for caller-supplied rays (integrators/mod.rs:94-101).  With `ray_counts`: (li, the closest-hit rays
        every sample traced (n,) uint32 — RadianceResult::ray_scene_intersections; Whitted only, zeros for Path, see yk_li)."""
        o = np.ascontiguousarray(ray_o, dtype=np.float32)
        d = np.ascontiguousarray(ray_d, dtype=np.float32)
        pix = np.ascontiguousarray(pixel_xy, dtype=np.uint16)
        si = np.ascontiguousarray(sample_index, dtype=np.uint32)
        out = np.zeros((o.shape[0], 3), dtype=np.float32)
        counts = np.zeros(o.shape[0], dtype=np.uint32) if ray_counts else None
        check(lib().yk_li(self.ctx.h, scene.h, C.byref(sampler), C.byref(self.desc), o.shape[0], _p(o), _p(d), _p(pix), _p(si), dimension, _p(out), _p(counts)), self.ctx.h)
        return (out, counts) if ray_counts else out

    def li_debug(self, scene, sampler, ray_o, ray_d, pixel_xy, sample_index, dimension=2):
        """Integrator::li_debug (integrators/mod.rs:103-115), Path only: returns (li (n,3), ray_counts (n,), rays), where
        rays[i] holds sample i's records (abi.INTEGRATOR_RAY_DTYPE, `ray_type` a RayType) in the reference's push order.
        The capacity is max_depth * (2 + lights), which always suffices."""
        cap = self.desc.max_depth * (2 + scene.n_lights)
        li, counts, recs, n_rays = self.li_debug_records(scene, sampler, ray_o, ray_d, pixel_xy, sample_index, dimension, cap)
        return li, counts, [recs[i, : n_rays[i]] for i in range(len(n_rays))]

    def li_debug_records(self, scene, sampler, ray_o, ray_d, pixel_xy, sample_index, dimension, ray_cap):
        """yk_li_debug as it is: (li, ray_counts, records (n, ray_cap), n_rays), where n_rays[i] may exceed ray_cap
        (then only the first ray_cap records of sample i were stored)."""
        o = np.ascontiguousarray(ray_o, dtype=np.float32)
        d = np.ascontiguousarray(ray_d, dtype=np.float32)
        pix = np.ascontiguousarray(pixel_xy, dtype=np.uint16)
        si = np.ascontiguousarray(sample_index, dtype=np.uint32)
        n = o.shape[0]
        out = np.zeros((n, 3), dtype=np.float32)
        counts = np.zeros(n, dtype=np.uint32)
        n_rays = np.zeros(n, dtype=np.uint32)
        recs = np.zeros((n, ray_cap), dtype=abi.INTEGRATOR_RAY_DTYPE)
        check(
            lib().yk_li_debug(self.ctx.h, scene.h, C.byref(sampler), C.byref(self.desc), n, _p(o), _p(d), _p(pix), _p(si), dimension, ray_cap, _p(out), _p(counts), _p(recs) if ray_cap else None, _p(n_rays)),
            self.ctx.h,
        )
        return out, counts, recs, n_rays


class IntegratorType:
    """integrators/mod.rs:33-53."""

    @staticmethod
    def Path(params: PathParams = None):
        params = params or PathParams()
        return abi.IntegratorDesc(abi.INTEGRATOR_PATH, params.max_depth, 0 if params.indirect_clamp is None else 1, 0.0 if params.indirect_clamp is None else params.indirect_clamp)

    @staticmethod
    def Whitted(max_depth=3):
        return abi.IntegratorDesc(abi.INTEGRATOR_WHITTED, max_depth, 0, 0.0)

    BVHIntersections = abi.IntegratorDesc(abi.INTEGRATOR_BVH_INTERSECTIONS, 1, 0, 0.0)
    GeometryNormals = abi.IntegratorDesc(abi.INTEGRATOR_GEOMETRY_NORMALS, 1, 0, 0.0)
    ShadingNormals = abi.IntegratorDesc(abi.INTEGRATOR_SHADING_NORMALS, 1, 0, 0.0)
    ShadingUVs = abi.IntegratorDesc(abi.INTEGRATOR_SHADING_UVS, 1, 0, 0.0)

    @staticmethod
    def instantiate(ctx, desc):
        return Integrator(ctx, desc)


# --------------------------------------------------------------------------- misc stage hooks
def device_math(ctx, fn, a, b=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    bb = None if b is None else np.ascontiguousarray(b, dtype=np.float32)
    out = np.zeros_like(a)
    check(lib().yk_device_math(ctx.h, fn, a.size, _p(a), _p(bb), _p(out)), ctx.h)
    return out


def host_math(fn, a, b=None):
    """yk_host_math: the host instance of yk_libm.h (no device needed)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    bb = None if b is None else np.ascontiguousarray(b, dtype=np.float32)
    out = np.zeros_like(a)
    check(lib().yk_host_math(fn, a.size, _p(a), _p(bb), _p(out)))
    return out


def sampler_sequence(ctx, sampler, px, py, sample_index, dims):
    dims = np.ascontiguousarray(dims, dtype=np.uint8)
    out = np.zeros((len(dims), 2), dtype=np.float32)
    check(lib().yk_sampler_sequence(ctx.h, C.byref(sampler), px, py, sample_index, _p(dims), len(dims), _p(out)), ctx.h)
    return out


def camera_rays(ctx, camera, sampler, tile, sample_index):
    t = abi.Tile(*[int(v) for v in tile])
    n = (t.x1 - t.x0) * (t.y1 - t.y0)
    o = np.zeros((n, 3), dtype=np.float32)
    d = np.zeros((n, 3), dtype=np.float32)
    check(lib().yk_camera_rays(ctx.h, C.byref(camera.matrices), C.byref(sampler), C.byref(t), sample_index, _p(o), _p(d)), ctx.h)
    return o, d


def bsdf_eval(ctx, material, n_geom, n_shading, dpdu, wo, wi):
    arrs = [np.ascontiguousarray(x, dtype=np.float32) for x in (n_geom, n_shading, dpdu, wo, wi)]
    out = np.zeros((arrs[0].shape[0], 3), dtype=np.float32)
    check(lib().yk_bsdf_eval(ctx.h, C.byref(material), arrs[0].shape[0], *[_p(x) for x in arrs], _p(out)), ctx.h)
    return out


def light_sample(ctx, light, light_index, p, n_geom, u):
    """Light::sample_li + VisibilityTester::ray on the device: (n, 18) floats, see yk_light_sample"""
    arrs = [np.ascontiguousarray(x, dtype=np.float32) for x in (p, n_geom, u)]
    out = np.zeros((arrs[0].shape[0], 18), dtype=np.float32)
    check(lib().yk_light_sample(ctx.h, C.byref(light), int(light_index), arrs[0].shape[0], *[_p(x) for x in arrs], _p(out)), ctx.h)
    return out


def surface(ctx, scene, ray_o, ray_d, route=0):
    """The SurfaceInteraction of the closest hit of n rays: (n, abi.SURFACE_FLOATS) floats, fields abi.SURFACE_FIELDS, see yk_surface.
    route 0: by leaf-order slot (the Path wavefront, debug integrators, guides); 1: by source shape (Whitted, li_debug)."""
    o = np.ascontiguousarray(ray_o, dtype=np.float32)
    d = np.ascontiguousarray(ray_d, dtype=np.float32)
    out = np.zeros((o.shape[0], abi.SURFACE_FLOATS), dtype=np.float32)
    check(lib().yk_surface(ctx.h, scene.h, o.shape[0], _p(o), _p(d), int(route), _p(out)), ctx.h)
    return out


def bsdf_sample(ctx, material, n_geom, n_shading, dpdu, wo, u):
    arrs = [np.ascontiguousarray(x, dtype=np.float32) for x in (n_geom, n_shading, dpdu, wo, u)]
    out = np.zeros((arrs[0].shape[0], 8), dtype=np.float32)
    check(lib().yk_bsdf_sample(ctx.h, C.byref(material), arrs[0].shape[0], *[_p(x) for x in arrs], _p(out)), ctx.h)
    return out
