#!/usr/bin/env python3
"""Device time of adaptive sampling on a 1080p film of cfg3 (Path depth 5), one MI355X:

  select    yk_adaptive_select_device at about 0 %, 10 %, 50 % and 100 % selected: device events around the call (the three
            launches and the 4-byte copy) and the host's wall clock around it; the difference is what the count's round trip
            costs beyond the kernels (one stream synchronisation per selection);
  fold      yk_adaptive_accumulate_device, 4 passes of a full list; resolve: yk_adaptive_resolve_device;
  render    samples per second of yk_render_pixel_list_device (4 passes) at 100 %, 50 % and 10 % occupancy, the pixels
            clustered (the first tiles of the list's order) or scattered (drawn at random, in the list's order), against
            yk_render_tile_list_samples_device on full passes of the same film in the same run: the yardstick.  Times are the
            calls' own device events (yk_render_stats.seconds_total);
  adaptive  one end-to-end figure: time and error of render_adaptive at the defaults under Uniform `--cap`, against uniform
            passes at ceil(mean spp) — error = RMSE of x / (1 + x) against `--reference-spp` samples a pixel.

Method of tools/variance_bench.py: `--warmup` calls, then `--launches` calls, medians with ranges.  The result is rewritten
after every stage, so a run that is cut short keeps what it measured.

    python tools/adaptive_bench.py --out profiles/adaptive_device.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yuki_amd import abi  # noqa: E402
from yuki_amd import core as yk  # noqa: E402
from yuki_amd import scenes  # noqa: E402

RES = (1920, 1080)
SEED = 0x73B9642E74AC471C
PASSES = 4


def summary(v, unit, **kw):
    return {f"min_{unit}": round(min(v), 2), f"median_{unit}": round(statistics.median(v), 2), f"max_{unit}": round(max(v), 2), "n": len(v), **kw}


def order_of_the_rule(w, h):
    """Every pixel as x | y << 16 in the order of the list: 16 x 16 tiles row-major, rows inside the clipped tile."""
    ys, xs = np.mgrid[0:h, 0:w]
    key = ((ys // 16) * ((w + 15) // 16) + xs // 16) * 256 + (ys % 16) * 16 + xs % 16
    o = np.argsort(key.reshape(-1), kind="stable")
    return (xs.reshape(-1)[o] | (ys.reshape(-1)[o] << 16)).astype(np.uint32)


def quality_error(x, ref_film):
    a, b = np.asarray(x, np.float64), np.asarray(ref_film, np.float64)
    d = a / (1.0 + a) - b / (1.0 + b)
    return float(np.sqrt(np.mean(d * d)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cfg3")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--renders", type=int, default=3)
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--reference-spp", type=int, default=256)
    ap.add_argument("--skip-adaptive", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    w, h = RES
    n_px = w * h
    ctx = yk.Context(0)
    sd = scenes.by_name(a.scene)
    fs = yk.FilmSettings(res=RES, tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    sc = yk.Scene(ctx, sd)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=5)))
    stream = torch.cuda.Stream()
    cs = stream.cuda_stream
    result = dict(tool="tools/adaptive_bench.py", film=list(RES), scene=a.scene, depth=5, warmup=a.warmup, launches=a.launches, passes=PASSES)

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")

    # ---- select
    rule = yk.AdaptiveParams(min_samples=16, max_samples=128, round_passes=16)
    pl = yk.PixelList(ctx, RES)
    rng = np.random.default_rng(1)
    result["select"] = {}
    for want in (0.0, 0.1, 0.5, 1.0):
        stats = np.zeros((h, w), dtype=abi.PIXEL_STATS_DTYPE)
        stats["n"] = stats["drawn"] = 16
        stats["mean"] = 1.0
        blocks = rng.random(((h + 7) // 8, (w + 7) // 8)) < want  # 8 x 8 blocks of wanting pixels: the dilation adds their rims
        stats["n"][np.kron(blocks, np.ones((8, 8), dtype=bool))[:h, :w]] = 0
        d_stats = torch.from_numpy(stats.view(np.int32).reshape(-1).copy()).to("cuda:0")
        torch.cuda.synchronize()
        ev_us, wall_us, count = [], [], 0
        for k in range(a.warmup + a.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            count = ctx.adaptive_select_device(d_stats.data_ptr(), RES, rule, pl, stream=cs)
            e1.record(stream)
            t1 = time.perf_counter()
            stream.synchronize()
            if k >= a.warmup:
                ev_us.append(e0.elapsed_time(e1) * 1e3)
                wall_us.append((t1 - t0) * 1e6)
        result["select"][f"{int(want * 100)}%"] = dict(selected=count, selected_fraction=round(count / n_px, 4), device=summary(ev_us, "us"), wall=summary(wall_us, "us"),
                                                       round_trip_us=round(statistics.median(wall_us) - statistics.median(ev_us), 2))  # fmt: skip
        print("select", want, result["select"][f"{int(want * 100)}%"], flush=True)
    save()

    # ---- fold and resolve on a full list
    full = order_of_the_rule(w, h)
    pl.set(full, np.zeros(n_px, np.uint32), passes=PASSES)
    d_passes = torch.rand(PASSES * n_px * 3, dtype=torch.float32, device="cuda:0")
    d_film = torch.zeros(n_px * 3, dtype=torch.float32, device="cuda:0")
    d_stats = torch.zeros(n_px * 4, dtype=torch.int32, device="cuda:0")
    d_rgb, d_var = torch.zeros(n_px * 3, dtype=torch.float32, device="cuda:0"), torch.zeros(n_px, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()

    def timed(call):
        for _ in range(a.warmup):
            call()
        stream.synchronize()
        events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
        for e0, e1 in events:
            e0.record(stream)
            call()
            e1.record(stream)
        stream.synchronize()
        return [e0.elapsed_time(e1) * 1e3 for e0, e1 in events]

    us = timed(lambda: ctx.adaptive_accumulate_device(pl, d_passes.data_ptr(), PASSES, RES, d_film.data_ptr(), d_stats.data_ptr(), stream=cs))
    moved = n_px * (4 + PASSES * 12 + 2 * 12 + 2 * 16)
    result["fold"] = summary(us, "us", bytes=moved, gbps=round(moved / statistics.median(us) * 1e-3, 1))
    us = timed(lambda: ctx.adaptive_resolve_device(d_film.data_ptr(), d_stats.data_ptr(), RES, d_rgb.data_ptr(), d_var.data_ptr(), stream=cs))
    result["resolve"] = summary(us, "us", bytes=n_px * 44, gbps=round(n_px * 44 / statistics.median(us) * 1e-3, 1))
    print("fold", result["fold"], "resolve", result["resolve"], flush=True)
    del d_passes
    save()

    # ---- list render against full passes of a tile list
    sampler = yk.SamplerType.Uniform(a.cap, SEED)
    tl = yk.TileList(ctx, yk.film_tiles(fs))
    slab = torch.zeros(PASSES * n_px * 3, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()

    def rate(call):
        r = []
        for k in range(1 + a.renders):
            st = call()
            if k:
                r.append(st.samples / st.seconds_total * 1e-6)
        return r

    tiles_rate = lambda: rate(lambda: it.render_tile_list_samples_device(sc, cam, sampler, tl, 0, PASSES, slab.data_ptr(), want_stats=True))  # noqa: E731
    result["render"] = dict(tile_list_full_passes=summary(tiles_rate(), "msamples_per_s"))
    print("tile list", result["render"]["tile_list_full_passes"], flush=True)
    for frac in (1.0, 0.5, 0.1):
        for how in ("clustered", "scattered"):
            if frac == 1.0 and how == "scattered":
                continue
            n = int(n_px * frac)
            xy = full[:n] if how == "clustered" else full[np.sort(rng.permutation(n_px)[:n])]
            pl.set(xy, np.zeros(n, np.uint32), passes=PASSES)
            r = rate(lambda: it.render_pixel_list_device(sc, cam, sampler, pl, PASSES, slab.data_ptr(), want_stats=True))
            result["render"][f"pixel_list_{int(frac * 100)}%_{how}"] = summary(r, "msamples_per_s", entries=n)
            print("pixel list", frac, how, result["render"][f"pixel_list_{int(frac * 100)}%_{how}"], flush=True)
    result["render"]["tile_list_full_passes_again"] = summary(tiles_rate(), "msamples_per_s")
    yard = statistics.median([result["render"]["tile_list_full_passes"]["median_msamples_per_s"], result["render"]["tile_list_full_passes_again"]["median_msamples_per_s"]])
    for k, v in result["render"].items():
        if k.startswith("pixel_list"):
            v["over_tile_list"] = round(v["median_msamples_per_s"] / yard, 3)
    del slab
    save()

    # ---- end to end
    if not a.skip_adaptive:
        p = yk.AdaptiveParams.for_sampler(sampler)
        film_tile = np.array([(0, 0, w, h)], dtype=abi.TILE_DTYPE)
        t0 = time.perf_counter()
        film, stats, info = it.render_adaptive(sc, cam, sampler, fs, p)
        torch.cuda.synchronize()
        t_adaptive = time.perf_counter() - t0
        ctx.adaptive_resolve_device(film.data_ptr(), stats.data_ptr(), RES, d_rgb.data_ptr(), None)
        torch.cuda.synchronize()
        rgb = d_rgb.cpu().numpy().reshape(h, w, 3)
        k = -(-int(info.samples) // n_px)
        acc = torch.zeros(n_px * 3, dtype=torch.float32, device="cuda:0")
        one = torch.zeros(n_px * 3, dtype=torch.float32, device="cuda:0")
        whole = yk.TileList(ctx, film_tile)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(k):
            it.render_tile_list_samples_device(sc, cam, sampler, whole, s, 1, one.data_ptr())
            whole.update_film_device(one.data_ptr(), RES, acc.data_ptr(), accumulate=True)
        torch.cuda.synchronize()
        t_uniform = time.perf_counter() - t0
        uniform = acc.cpu().numpy().reshape(h, w, 3) / k
        ref_sampler = yk.SamplerType.Uniform(a.reference_spp, SEED ^ 0x1234567)
        acc.zero_()
        torch.cuda.synchronize()
        for s in range(a.reference_spp):
            it.render_tile_list_samples_device(sc, cam, ref_sampler, whole, s, 1, one.data_ptr())
            whole.update_film_device(one.data_ptr(), RES, acc.data_ptr(), accumulate=True)
        torch.cuda.synchronize()
        conv = acc.cpu().numpy().reshape(h, w, 3) / a.reference_spp
        e_ad, e_un = quality_error(rgb, conv), quality_error(uniform, conv)
        result["adaptive"] = dict(cap=a.cap, reference_spp=a.reference_spp, params=dict(min_samples=p.min_samples, round_passes=p.round_passes, threshold=p.threshold, epsilon=p.epsilon, dilate=int(p.dilate)),
                                  rounds=info.rounds, converged=info.converged, mean_spp=round(info.samples / n_px, 2), first_pixels=info.first_pixels, last_pixels=info.last_pixels,
                                  seconds_adaptive=round(t_adaptive, 4), uniform_spp=k, seconds_uniform=round(t_uniform, 4), e_adaptive=round(e_ad, 5), e_uniform=round(e_un, 5), ratio=round(e_ad / e_un, 4))  # fmt: skip
        print("adaptive", result["adaptive"], flush=True)
        whole.close()
        save()
    tl.close()
    pl.close()
    sc.close()
    ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
