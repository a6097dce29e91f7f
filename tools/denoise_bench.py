#!/usr/bin/env python3
"""Device time of the denoiser (yk_denoise_device, k_atrous) on a 1080p film, per iteration and per kernel variant, and
of the guide pass (yk_render_guides_device), from device events.

The film is cfg3 at 1080p, Path depth 5, 4 samples a pixel, rendered by the device; the guides are its own.  A denoise of
k iterations is k launches enqueued by one call, so an iteration is timed as a difference: after `--warmup` calls,
`--launches` calls of k iterations for k = 1 .. 5, each between its own pair of events on the caller's stream; iteration
i costs median(k = i + 1) - median(k = i).  (The last launch of a call writes 12 bytes a pixel instead of 16, so the
difference is a few per cent kind to the later iteration.)  That is done with "denoise_lds_max_step" 0 (every tap from
global memory) and 2 (steps 1 and 2 staged in LDS); the results of the two settings are compared bit for bit.
Recorded too: the bytes an iteration must at least move (16 + 32 read and 16 written per pixel), the rate that gives
against the 6.29 TB/s copy ceiling, and, for scale, the accumulating pass the denoiser sits beside.

    python tools/denoise_bench.py --out profiles/denoise_device.json
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

COPY_CEILING_GBPS = 6290.0  # the measured copy ceiling of the MI355X the project compares with
ACCUMULATING_PASS_MS = 7.0  # one 1080p accumulating pass of a GPU worker
RES = (1920, 1080)
ITERATIONS = 5
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cfg3")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = yk.Context(0)
    sd = scenes.by_name(a.scene)
    fs = yk.FilmSettings(res=RES, tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    sc = yk.Scene(ctx, sd)
    tiles = yk.film_tiles(fs)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=5)))
    film = yk.update_tiles(tiles, it.render_tiles(sc, cam, yk.SamplerType.Uniform(4, SEED), tiles)[0], fs.res)
    params = yk.DenoiseParams.for_scene(sc, iterations=ITERATIONS)
    n_px = RES[0] * RES[1]
    stream = torch.cuda.Stream()
    d_film = torch.from_numpy(film.reshape(-1)).to("cuda:0")
    d_guides = torch.zeros(n_px * 8, dtype=torch.float32, device="cuda:0")
    d_out = torch.zeros_like(d_film)
    torch.cuda.synchronize()

    us = timed(stream, a.launches, a.warmup, lambda: ctx.render_guides_device(sc, cam, RES, d_guides.data_ptr(), stream=stream.cuda_stream))
    hit = float((d_guides.view(-1, 8)[:, 3] != 0).float().mean().item())
    guides = dict(scene=a.scene, launch_us=[round(t, 2) for t in us], min_us=round(min(us), 2), median_us=round(statistics.median(us), 2), max_us=round(max(us), 2), hit_fraction=round(hit, 4))
    print("render_guides_device", json.dumps({k: v for k, v in guides.items() if k != "launch_us"}), flush=True)

    moved = n_px * (16 + 32 + 16)
    variants, outputs = {}, {}
    for lds_max_step in (0, 2):
        ctx.set_option("denoise_lds_max_step", lds_max_step)
        prefix = []
        for k in range(1, ITERATIONS + 1):
            p = yk.DenoiseParams(k, params.sigma_color, params.sigma_normal, params.sigma_plane)
            t = timed(stream, a.launches, a.warmup, lambda: ctx.denoise_device(d_film.data_ptr(), d_guides.data_ptr(), RES, p, 16, None, d_out.data_ptr(), stream=stream.cuda_stream))
            prefix.append(dict(iterations=k, launch_us=[round(v, 2) for v in t], min_us=round(min(t), 2), median_us=round(statistics.median(t), 2), max_us=round(max(t), 2)))
        outputs[lds_max_step] = d_out.cpu().numpy().copy()
        per_iteration = []
        for i in range(ITERATIONS):
            dt = prefix[i]["median_us"] - (prefix[i - 1]["median_us"] if i else 0.0)
            kernel = "lds" if (1 << i) <= lds_max_step else "global"
            per_iteration.append(dict(iteration=i, step=1 << i, kernel=kernel, us=round(dt, 2), gbps=round(moved / dt * 1e-3, 1), share_of_copy_ceiling=round(moved / dt * 1e-3 / COPY_CEILING_GBPS, 3)))
        variants[f"lds_max_step_{lds_max_step}"] = dict(calls=prefix, per_iteration=per_iteration, total_us=prefix[-1]["median_us"])
        print(f"lds_max_step {lds_max_step}", json.dumps(per_iteration), "total", prefix[-1]["median_us"], flush=True)
    equal = bool(np.array_equal(outputs[0].view(np.uint32), outputs[2].view(np.uint32)))
    result = dict(tool="tools/denoise_bench.py", timing="device events around each call; an iteration is the difference of the medians of k + 1 and k iterations",
                  film=list(RES), scene=a.scene, iterations=ITERATIONS, warmup=a.warmup, launches=a.launches, params=dict(sigma_color=params.sigma_color, sigma_normal=params.sigma_normal, sigma_plane=params.sigma_plane),
                  copy_ceiling_gbps=COPY_CEILING_GBPS, min_bytes_per_iteration=moved, accumulating_pass_ms=ACCUMULATING_PASS_MS, render_guides_device=guides, denoise=variants, variants_equal_bit_for_bit=equal)
    print("variants equal bit for bit:", equal, flush=True)
    sc.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    assert equal, "the two kernel variants differ"


if __name__ == "__main__":
    main()
