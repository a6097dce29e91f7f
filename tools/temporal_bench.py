#!/usr/bin/env python3
"""Device time of the temporal passes (yk_history_reproject_device: k_reproject, yk_history_blend_device: k_record_blend) on a
1080p film, from device events.

The scene is cfg3 at 1080p.  Camera A is the scene's own, camera B the same camera a small orbit step (`--orbit-degrees`
about the up axis through the target) further.  The history is the blend of a one-sample film the device rendered at A;
the guides of both views are the device's.  After `--warmup` calls, `--launches` calls of each pass, each between its own
pair of events on the caller's stream; reported are the median and the range.  Blend is timed in its fullest form: a
sample table, a history, both outputs.
The calls repeat on the same buffers (199 MB for reproject), which fit in the 256 MB last-level cache: the times are
cache-warm, as they largely are in use, where the guides and the history were written just before.
Recorded beside each time: the bytes the pass must at least move and what they take at the 6.29 TB/s copy ceiling.
  reproject: 32 bytes of guide read, 48 bytes of previous record read (one tap's worth: the other three are a neighbour's)
             and 16 bytes written per pixel;
  blend:     12 + 16 bytes read and 16 + 12 written per pixel.

    python tools/temporal_bench.py --out profiles/temporal_device.json
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yuki_amd import core as yk  # noqa: E402
from yuki_amd import scenes  # noqa: E402

COPY_CEILING_GBPS = 6290.0  # the measured copy ceiling of the MI355X the project compares with
ACCUMULATING_PASS_MS = 7.0  # one 1080p accumulating pass of a GPU worker
RES = (1920, 1080)
SEED = 0x73B9642E74AC471C


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


def orbit(cam, degrees):
    """The camera turned about the up axis (y) through its target."""
    p, t = np.array(cam["position"], np.float64), np.array(cam["target"], np.float64)
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    d = p - t
    return dict(cam, position=tuple(t + np.array([c * d[0] + s * d[2], d[1], -s * d[0] + c * d[2]])))


def summary(us, moved):
    med = statistics.median(us)
    floor_us = moved / COPY_CEILING_GBPS * 1e-3
    return dict(launch_us=[round(t, 2) for t in us], min_us=round(min(us), 2), median_us=round(med, 2), max_us=round(max(us), 2), min_bytes=moved, floor_us=round(floor_us, 2),
                gbps=round(moved / med * 1e-3, 1), share_of_copy_ceiling=round(floor_us / med, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cfg3")
    ap.add_argument("--orbit-degrees", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = yk.Context(0)
    sd = scenes.by_name(a.scene)
    fs = yk.FilmSettings(res=RES, tile_dim=16)
    cam_a, cam_b = yk.Camera(sd.camera, fs), yk.Camera(orbit(sd.camera, a.orbit_degrees), fs)
    sc = yk.Scene(ctx, sd)
    tiles = yk.film_tiles(fs)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=5)))
    film = yk.update_tiles(tiles, it.render_tiles(sc, cam_a, yk.SamplerType.Uniform(1, SEED), tiles)[0], fs.res)
    params = yk.TemporalParams.for_scene(sc)
    n_px = RES[0] * RES[1]
    samples = np.ones((-(-RES[0] // 16)) * (-(-RES[1] // 16)), np.uint32)
    stream = torch.cuda.Stream()
    cs = stream.cuda_stream
    z = lambda k: torch.zeros(k, dtype=torch.float32, device="cuda:0")  # noqa: E731
    d_film = torch.from_numpy(film.reshape(-1)).to("cuda:0")
    d_ga, d_gb, d_hist_a, d_carried, d_hist_b, d_rgb = z(8 * n_px), z(8 * n_px), z(4 * n_px), z(4 * n_px), z(4 * n_px), z(3 * n_px)
    torch.cuda.synchronize()
    ctx.render_guides_device(sc, cam_a, RES, d_ga.data_ptr(), stream=cs)
    ctx.render_guides_device(sc, cam_b, RES, d_gb.data_ptr(), stream=cs)
    ctx.blend_history_device(d_film.data_ptr(), RES, params, 16, samples, None, d_hist_a.data_ptr(), None, stream=cs)
    stream.synchronize()

    us = timed(stream, a.launches, a.warmup, lambda: ctx.reproject_history_device(d_hist_a.data_ptr(), d_ga.data_ptr(), cam_a, d_gb.data_ptr(), RES, params, d_carried.data_ptr(), stream=cs))
    reproject = summary(us, n_px * (32 + 48 + 16))
    hit = float((d_gb.view(-1, 8)[:, 3] != 0).float().mean().item())
    reused = float((d_carried.view(-1, 4)[:, 3] > 0).float().mean().item())
    reproject.update(hit_fraction=round(hit, 4), pixels_with_history=round(reused, 4))
    print("reproject", json.dumps({k: v for k, v in reproject.items() if k != "launch_us"}), flush=True)

    us = timed(stream, a.launches, a.warmup, lambda: ctx.blend_history_device(d_film.data_ptr(), RES, params, 16, samples, d_carried.data_ptr(), d_hist_b.data_ptr(), d_rgb.data_ptr(), stream=cs))
    blend = summary(us, n_px * (12 + 16 + 16 + 12))
    print("blend", json.dumps({k: v for k, v in blend.items() if k != "launch_us"}), flush=True)

    result = dict(tool="tools/temporal_bench.py", timing="device events around each call", film=list(RES), scene=a.scene, orbit_degrees=a.orbit_degrees, warmup=a.warmup, launches=a.launches,
                  params=dict(plane_tolerance=params.plane_tolerance, normal_cos_min=params.normal_cos_min, max_history=params.max_history), copy_ceiling_gbps=COPY_CEILING_GBPS,
                  accumulating_pass_ms=ACCUMULATING_PASS_MS, reproject=reproject, blend=blend)
    sc.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
