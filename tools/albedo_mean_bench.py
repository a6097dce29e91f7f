#!/usr/bin/env python3
"""Device time of the pixel-mean albedo on a 1080p film, from device events: the fused route yk_render_albedo_mean_device
(the large film traced in bands and reduced, never whole) for s = 2 and s = 4 under several band sizes, and the reduction
alone (yk_albedo_mean_device, k_albedo_mean) on the whole large film's ids.

The scene is cfg3 with its ground textured by a 256 x 256 image, as in tools/albedo_bench.py.  The yardstick is the pair
yk_render_guides_ids_device (ids only) + yk_surface_albedo_device at 1080p, timed in the same run before and after
everything else: the fused time is reported as a multiple of s*s times that pair.  Method of tools/albedo_bench.py: after
`--warmup` calls, `--launches` calls, each between its own pair of events on the caller's stream; medians with ranges.
Each fused result is compared bit for bit with the reduction of the whole large film's ids.

    python tools/albedo_mean_bench.py --out profiles/albedo_mean_device.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yuki_amd import abi  # noqa: E402
from yuki_amd import core as yk  # noqa: E402
from yuki_amd import scenes  # noqa: E402

RES = (1920, 1080)
BANDS = {2: (68, 135, 270, 0, 1080), 4: (17, 34, 68, 0, 270, 1080)}  # output rows per band; 0 = the library's default


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
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = yk.Context(0)
    sd = scenes.by_name(a.scene)
    sd.materials[len(sd.materials) - 2] = dict(kind=abi.MAT_MATTE, a=(0.55, 0.55, 0.55), c=0.0, tex=0)
    sd.textures = [(0.1 + 0.8 * np.random.default_rng(3).random((256, 256, 3))).astype(np.float32)]
    fs = yk.FilmSettings(res=RES, tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    sc = yk.Scene(ctx, sd)
    n_px = RES[0] * RES[1]
    stream = torch.cuda.Stream()
    cs = stream.cuda_stream
    d_ids = torch.zeros(4 * n_px, dtype=torch.int32, device="cuda:0")
    d_albedo, d_mean, d_want = (torch.zeros(4 * n_px, dtype=torch.float32, device="cuda:0") for _ in range(3))
    torch.cuda.synchronize()
    result = dict(tool="tools/albedo_mean_bench.py", timing="device events around each call", film=list(RES), scene=a.scene, texture=[256, 256], warmup=a.warmup, launches=a.launches)

    def pair():
        ctx.render_guides_ids_device(sc, cam, RES, None, d_ids.data_ptr(), stream=cs)
        ctx.surface_albedo_device(sc, d_ids.data_ptr(), RES, d_albedo.data_ptr(), stream=cs)

    result["pair_before"] = summary(timed(stream, a.launches, a.warmup, pair))
    print("pair (ids + centre albedo at 1080p)", result["pair_before"]["median_us"], flush=True)
    pair_us = result["pair_before"]["median_us"]
    for s, bands in BANDS.items():
        big = (s * RES[0], s * RES[1])
        cam_ss = yk.Camera(sd.camera, yk.supersampled(fs, s))
        d_ids_ss = torch.zeros(4 * n_px * s * s, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        us = timed(stream, a.launches, a.warmup, lambda: ctx.render_guides_ids_device(sc, cam_ss, big, None, d_ids_ss.data_ptr(), stream=cs))
        result[f"s{s}_render_ids_whole_large_film"] = summary(us, res=list(big), bytes=16 * n_px * s * s)
        us = timed(stream, a.launches, a.warmup, lambda: ctx.albedo_mean_device(sc, d_ids_ss.data_ptr(), RES, s, d_want.data_ptr(), stream=cs))
        moved = n_px * (16 * s * s + 16)
        result[f"s{s}_reduction_alone"] = summary(us, min_bytes=moved, gbps=round(moved / statistics.median(us) * 1e-3, 1))
        print(f"s={s}: ids of the whole large film {result[f's{s}_render_ids_whole_large_film']['median_us']}, reduction alone {result[f's{s}_reduction_alone']['median_us']}", flush=True)
        want = d_want.cpu().numpy().view(np.uint32).copy()
        known = float((d_want.view(-1, 4)[:, 3] != 0).float().mean().item())
        for rows in bands:
            ctx.set_option("albedo_mean_band_rows", rows)
            us = timed(stream, a.launches, a.warmup, lambda: ctx.render_albedo_mean_device(sc, cam_ss, RES, s, d_mean.data_ptr(), stream=cs))
            same = bool(np.array_equal(d_mean.cpu().numpy().view(np.uint32), want))
            med = statistics.median(us)
            result[f"s{s}_fused_band_{rows if rows else 'default'}"] = summary(us, band_rows=rows, over_s2_pairs=round(med / (s * s * pair_us), 3), equals_reduction_of_whole_film=same, known_fraction=round(known, 4))
            print(f"s={s} band {rows if rows else 'default'}: {round(med, 1)} us = {round(med / (s * s * pair_us), 3)} x s^2 pairs, bit-identical {same}", flush=True)
        ctx.set_option("albedo_mean_band_rows", 0)
        del d_ids_ss
        torch.cuda.empty_cache()
    result["pair_after"] = summary(timed(stream, a.launches, a.warmup, pair))
    print("pair again", result["pair_after"]["median_us"], flush=True)
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
