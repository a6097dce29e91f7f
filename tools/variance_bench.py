#!/usr/bin/env python3
"""Device time of the variance-guided denoise on a 1080p film, from device events: yk_moments_blend_device,
yk_variance_device with every pixel on the temporal estimate and with every pixel on the spatial one, and a 5-iteration
yk_denoise_variance_device with and without an albedo — against plain yk_denoise_device in the same run on the same box,
which is the yardstick.

The film is cfg3 at 1080p, Path depth 5, two frames of 4 samples a pixel rendered by the device and folded by
blend_history_device / blend_moments_device; guides, ids and albedo are its own; both filters run 5 iterations at the
library's defaults and "denoise_lds_max_step".  Method of tools/albedo_bench.py: after `--warmup` calls, `--launches`
calls, each between its own pair of events on the caller's stream; medians with ranges; plain denoise is timed before and
after the new calls, so that a drift of the clocks does not read as a difference.  Per iteration both filters move the same
64 bytes a pixel; the new one adds the preparing pass (12 + 4 read, 16 written).

    python tools/variance_bench.py --out profiles/variance_device.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yuki_amd import core as yk  # noqa: E402
from yuki_amd import scenes  # noqa: E402

RES = (1920, 1080)
ITERATIONS = 5
SEED = 0x73B9642E74AC471C
PARENT_PLAIN_US = dict(albedo_device=(721.21, 795.57))  # profiles/albedo_device.json: the range of plain denoise over its three series


def timed(stream, launches, warmup, call):
    for _ in range(warmup):
        call()
    stream.synchronize()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in events:
        a.record(stream)
        call()
        b.record(stream)
    stream.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in events]


def summary(us, **kw):
    return dict(launch_us=[round(t, 2) for t in us], min_us=round(min(us), 2), median_us=round(statistics.median(us), 2), max_us=round(max(us), 2), **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cfg3")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--lds-max-step", type=int, default=None, help='"denoise_lds_max_step" (0, 1 or 2) instead of the library\'s default')
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = yk.Context(0)
    if a.lds_max_step is not None:
        ctx.set_option("denoise_lds_max_step", a.lds_max_step)
    sd = scenes.by_name(a.scene)
    fs = yk.FilmSettings(res=RES, tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    sc = yk.Scene(ctx, sd)
    tiles = yk.film_tiles(fs)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=5)))
    frames = [yk.update_tiles(tiles, it.render_tiles(sc, cam, yk.SamplerType.Uniform(4, SEED + 977 * k), tiles)[0], fs.res) for k in range(2)]
    plain_params = yk.DenoiseParams.for_scene(sc, iterations=ITERATIONS)
    vpar = yk.VarianceParams.for_scene(sc, iterations=ITERATIONS)
    tp = yk.TemporalParams.for_scene(sc)
    n_px = RES[0] * RES[1]
    stream = torch.cuda.Stream()
    cs = stream.cuda_stream
    z = lambda k: torch.zeros(k, dtype=torch.float32, device="cuda:0")  # noqa: E731
    d_frames = [torch.from_numpy(f.reshape(-1)).to("cuda:0") for f in frames]
    d_guides, d_ids, d_albedo, d_out = z(8 * n_px), z(4 * n_px), z(4 * n_px), z(3 * n_px)
    d_hist, d_mom, d_mom2, d_rgb, d_var = z(4 * n_px), z(4 * n_px), z(4 * n_px), z(3 * n_px), z(n_px)
    torch.cuda.synchronize()
    ctx.render_guides_ids_device(sc, cam, RES, d_guides.data_ptr(), d_ids.data_ptr(), stream=cs)
    ctx.surface_albedo_device(sc, d_ids.data_ptr(), RES, d_albedo.data_ptr(), stream=cs)
    ctx.blend_history_device(d_frames[0].data_ptr(), RES, tp, 16, None, None, d_hist.data_ptr(), d_rgb.data_ptr(), stream=cs)
    ctx.blend_moments_device(d_frames[0].data_ptr(), RES, tp, 16, None, None, d_mom.data_ptr(), stream=cs)
    ctx.blend_history_device(d_frames[1].data_ptr(), RES, tp, 16, None, d_hist.data_ptr(), d_hist.data_ptr(), d_rgb.data_ptr(), stream=cs)
    stream.synchronize()
    result = dict(tool="tools/variance_bench.py", timing="device events around each call", film=list(RES), scene=a.scene, iterations=ITERATIONS, warmup=a.warmup, launches=a.launches, lds_max_step=a.lds_max_step,
                  params=dict(sigma_variance=vpar.sigma_variance, sigma_normal=vpar.sigma_normal, sigma_plane=vpar.sigma_plane, epsilon=vpar.epsilon, spatial_scale=vpar.spatial_scale,
                              plain_sigma_color=plain_params.sigma_color))  # fmt: skip

    film, guides, rgb, var, out, albedo = (t.data_ptr() for t in (d_frames[1], d_guides, d_rgb, d_var, d_out, d_albedo))
    plain = lambda: ctx.denoise_device(rgb, guides, RES, plain_params, 16, None, out, stream=cs)  # noqa: E731
    result["denoise_plain"] = summary(timed(stream, a.launches, a.warmup, plain))
    print("denoise_plain", result["denoise_plain"]["median_us"], flush=True)
    us = timed(stream, a.launches, a.warmup, lambda: ctx.blend_moments_device(film, RES, tp, 16, None, d_mom.data_ptr(), d_mom2.data_ptr(), stream=cs))
    result["moments_blend_device"] = summary(us, bytes=n_px * 44, gbps=round(n_px * 44 / statistics.median(us) * 1e-3, 1))
    print("moments_blend_device", result["moments_blend_device"]["median_us"], flush=True)
    us = timed(stream, a.launches, a.warmup, lambda: ctx.variance_device(d_mom2.data_ptr(), rgb, guides, RES, vpar, 16, None, var, stream=cs))
    stream.synchronize()
    frames_ge_2 = float((d_mom2.view(-1, 4)[:, 2] >= 2).float().mean().item())
    result["variance_device_temporal"] = summary(us, temporal_fraction=round(frames_ge_2, 4), bytes=n_px * 20, gbps=round(n_px * 20 / statistics.median(us) * 1e-3, 1))
    print("variance_device (temporal)", result["variance_device_temporal"]["median_us"], "fraction", frames_ge_2, flush=True)
    us = timed(stream, a.launches, a.warmup, lambda: ctx.variance_device(None, rgb, guides, RES, vpar, 16, None, var, stream=cs))
    result["variance_device_spatial"] = summary(us)
    print("variance_device (spatial)", result["variance_device_spatial"]["median_us"], flush=True)
    ctx.variance_device(d_mom2.data_ptr(), rgb, guides, RES, vpar, 16, None, var, stream=cs)  # what the filter is timed on
    guided = lambda: ctx.denoise_variance_device(rgb, guides, var, RES, vpar, 16, None, out, stream=cs)  # noqa: E731
    guided_albedo = lambda: ctx.denoise_variance_device(rgb, guides, var, RES, vpar, 16, None, out, stream=cs, albedo=albedo)  # noqa: E731
    us = timed(stream, a.launches, a.warmup, guided)
    us_albedo = timed(stream, a.launches, a.warmup, guided_albedo)
    plain_again = timed(stream, a.launches, a.warmup, plain)
    result["denoise_plain_again"] = summary(plain_again)
    yard = statistics.median(result["denoise_plain"]["launch_us"] + [round(t, 2) for t in plain_again])
    result["denoise_variance"] = summary(us, over_plain=round(statistics.median(us) / yard, 3))
    result["denoise_variance_albedo"] = summary(us_albedo, over_plain=round(statistics.median(us_albedo) / yard, 3))
    print("denoise_variance", result["denoise_variance"]["median_us"], "with albedo", result["denoise_variance_albedo"]["median_us"], "plain", yard, flush=True)
    lo = min(result["denoise_plain"]["min_us"], result["denoise_plain_again"]["min_us"])
    hi = max(result["denoise_plain"]["max_us"], result["denoise_plain_again"]["max_us"])
    p_lo, p_hi = PARENT_PLAIN_US["albedo_device"]
    result["plain_against_parent"] = dict(parent_range_us=[p_lo, p_hi], this_range_us=[lo, hi], ranges_overlap=bool(lo <= p_hi and p_lo <= hi))
    guided()
    stream.synchronize()
    a_out = d_out.cpu().numpy().copy()
    plain()
    stream.synchronize()
    result["differs_from_plain"] = bool(not np.array_equal(a_out.view(np.uint32), d_out.cpu().numpy().view(np.uint32)))
    sc.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps({k: (v if not isinstance(v, dict) else {kk: vv for kk, vv in v.items() if kk != "launch_us"}) for k, v in result.items()}), flush=True)


if __name__ == "__main__":
    main()
