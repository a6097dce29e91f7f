#!/usr/bin/env python3
"""Device time of the albedo passes on a 1080p film, from device events: yk_surface_albedo_device (k_albedo),
yk_denoise_albedo_device against plain yk_denoise_device, and what the surface ids cost on top of the guide pass.

The film is cfg3 at 1080p, Path depth 5, 4 samples a pixel, rendered by the device; guides and ids are its own; the
denoiser runs 5 iterations at the library's default sigmas and "denoise_lds_max_step".  Method of tools/denoise_bench.py:
after `--warmup` calls, `--launches` calls, each between its own pair of events on the caller's stream; medians with
ranges.  The demodulated denoise moves 60 bytes a pixel more than the plain one (the preparing pass reads 12 + 16 and
writes 16, the last iteration reads 16 more): the added time is reported with its fraction of that traffic at the
6.29 TB/s copy ceiling.  k_albedo is timed on cfg3 as it is (no textures: three hops) and with its ground textured by a
256 x 256 image (four hops).

    python tools/albedo_bench.py --out profiles/albedo_device.json
    python tools/albedo_bench.py --plain-only --out plain.json     # another build of the library (YK_LIB_PATH): plain yk_denoise_device alone
    python tools/albedo_bench.py --other-plain plain.json --out profiles/albedo_device.json   # ... quoted beside this build's
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

COPY_CEILING_GBPS = 6290.0  # the measured copy ceiling of the MI355X the project compares with
K_MOTION_US = 23.0  # profiles/motion_device.json: the same kind of gather
RES = (1920, 1080)
ITERATIONS = 5
ADDED_BYTES_PER_PIXEL = 12 + 16 + 16 + 16
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


def summary(us, **kw):
    return dict(launch_us=[round(t, 2) for t in us], min_us=round(min(us), 2), median_us=round(statistics.median(us), 2), max_us=round(max(us), 2), **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cfg3")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--plain-only", action="store_true", help="time plain yk_denoise_device alone (a build without the albedo passes)")
    ap.add_argument("--other-plain", default="", help="the --plain-only result of another build, quoted beside this one's")
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
    film = yk.update_tiles(tiles, it.render_tiles(sc, cam, yk.SamplerType.Uniform(4, SEED), tiles)[0], fs.res)
    params = yk.DenoiseParams.for_scene(sc, iterations=ITERATIONS)
    n_px = RES[0] * RES[1]
    stream = torch.cuda.Stream()
    cs = stream.cuda_stream
    z = lambda k: torch.zeros(k, dtype=torch.float32, device="cuda:0")  # noqa: E731
    d_film = torch.from_numpy(film.reshape(-1)).to("cuda:0")
    d_guides, d_ids, d_albedo, d_out = z(8 * n_px), z(4 * n_px), z(4 * n_px), z(3 * n_px)
    torch.cuda.synchronize()
    result = dict(tool="tools/albedo_bench.py", timing="device events around each call", film=list(RES), scene=a.scene, iterations=ITERATIONS, warmup=a.warmup, launches=a.launches, lds_max_step=a.lds_max_step,
                  params=dict(sigma_color=params.sigma_color, sigma_normal=params.sigma_normal, sigma_plane=params.sigma_plane), copy_ceiling_gbps=COPY_CEILING_GBPS)

    us = timed(stream, a.launches, a.warmup, lambda: ctx.render_guides_device(sc, cam, RES, d_guides.data_ptr(), stream=cs))
    result["render_guides_device"] = summary(us)
    plain = lambda: ctx.denoise_device(d_film.data_ptr(), d_guides.data_ptr(), RES, params, 16, None, d_out.data_ptr(), stream=cs)  # noqa: E731
    result["denoise_plain"] = summary(timed(stream, a.launches, a.warmup, plain))
    print("denoise_plain", result["denoise_plain"]["min_us"], result["denoise_plain"]["median_us"], result["denoise_plain"]["max_us"], flush=True)
    if not a.plain_only:
        us = timed(stream, a.launches, a.warmup, lambda: ctx.render_guides_ids_device(sc, cam, RES, d_guides.data_ptr(), d_ids.data_ptr(), stream=cs))
        g = result["render_guides_device"]["median_us"]
        result["render_guides_ids_device"] = summary(us, over_guides=round(statistics.median(us) / g - 1.0, 4))
        us = timed(stream, a.launches, a.warmup, lambda: ctx.surface_albedo_device(sc, d_ids.data_ptr(), RES, d_albedo.data_ptr(), stream=cs))
        known = float((d_albedo.view(-1, 4)[:, 3] != 0).float().mean().item())
        moved = n_px * 32
        result["surface_albedo_device"] = summary(us, known_fraction=round(known, 4), k_motion_us=K_MOTION_US, min_bytes=moved, gbps=round(moved / statistics.median(us) * 1e-3, 1))
        print("surface_albedo_device", result["surface_albedo_device"]["median_us"], "known", known, flush=True)
        demod = lambda: ctx.denoise_device(d_film.data_ptr(), d_guides.data_ptr(), RES, params, 16, None, d_out.data_ptr(), stream=cs, albedo=d_albedo.data_ptr())  # noqa: E731
        # interleaved a second time, so that a drift of the clocks does not read as a difference
        plain_again = timed(stream, a.launches, a.warmup, plain)
        us = timed(stream, a.launches, a.warmup, demod)
        added = statistics.median(us) - statistics.median(plain_again)
        bound = n_px * ADDED_BYTES_PER_PIXEL / COPY_CEILING_GBPS * 1e-3
        result["denoise_plain_again"] = summary(plain_again)
        result["denoise_albedo"] = summary(us, added_us=round(added, 2), added_bytes=n_px * ADDED_BYTES_PER_PIXEL, bound_us=round(bound, 2), bound_over_added=round(bound / added, 3) if added > 0 else None)
        print("denoise_albedo", result["denoise_albedo"]["median_us"], "added", round(added, 2), "bound", round(bound, 2), flush=True)
        # bit for bit against the host instance on a corner of the film would need the whole film: the suite does that; here
        # only that the pass did something and an all-ones albedo is the plain filter
        demod()
        stream.synchronize()
        with_albedo = d_out.cpu().numpy().copy()
        plain()
        stream.synchronize()
        without = d_out.cpu().numpy().copy()
        d_albedo.view(-1, 4)[:, :3] = 1.0
        demod()
        stream.synchronize()
        result["differs_from_plain"] = bool(not np.array_equal(with_albedo.view(np.uint32), without.view(np.uint32)))
        result["ones_equal_plain_bit_for_bit"] = bool(np.array_equal(d_out.cpu().numpy().view(np.uint32), without.view(np.uint32)))
        sc.close()
        # the texel hop: the same scene with its ground (the second to last material) textured
        sd.materials[len(sd.materials) - 2] = dict(kind=abi.MAT_MATTE, a=(0.55, 0.55, 0.55), c=0.0, tex=0)
        sd.textures = [(0.1 + 0.8 * np.random.default_rng(3).random((256, 256, 3))).astype(np.float32)]
        sc = yk.Scene(ctx, sd)
        ctx.render_guides_ids_device(sc, cam, RES, d_guides.data_ptr(), d_ids.data_ptr(), stream=cs)
        us = timed(stream, a.launches, a.warmup, lambda: ctx.surface_albedo_device(sc, d_ids.data_ptr(), RES, d_albedo.data_ptr(), stream=cs))
        result["surface_albedo_device_textured_ground"] = summary(us, texture=[256, 256])
        print("surface_albedo_device (textured ground)", result["surface_albedo_device_textured_ground"]["median_us"], flush=True)
        if a.other_plain:
            with open(a.other_plain) as f:
                other = json.load(f)["denoise_plain"]
            mine = result["denoise_plain"]
            result["denoise_plain_other_build"] = dict(other, ranges_overlap=bool(mine["min_us"] <= other["max_us"] and other["min_us"] <= mine["max_us"]))
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
