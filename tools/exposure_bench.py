#!/usr/bin/env python3
"""Device time of the exposure meter (yk_exposure_meter_device: k_meter_hist + k_meter_final) and of the metered tone map
against the passes they sit beside, on device-resident films at 1080p and 3840 x 2160.

Baseline: the auto-bounds reduction the tone map already had (k_min_max_partial + k_min_max_final, reached through a
Heatmap without bounds), which reads the same 12 bytes a pixel, on the same film in the same run.

Films: log-uniform noise over 20 stops; a rendered cfg3 frame (Path depth 5, one sample a pixel); a constant film (one bin:
the contention case); a film whose upper half is black.  Each is metered with "exposure_wave_combine" 1 (the default) and 0.

Method of tools/denoise_bench.py: the films stay on the device and are small enough to stay in the Infinity Cache
(cache-warm, as a frame that was just written is); after `--warmup` calls, `--launches` calls per variant, the variants
alternating, `--rounds` times over.
  - Whole calls: device events around each call on the caller's stream, in this process.
  - Kernels: a run of its own — this script again as a fresh child process under `rocprofv3 --kernel-trace --stats`, doing
    the same sequence without events; the per-dispatch rows of its kernel trace are matched to the sequence by order.

    python tools/exposure_bench.py --out profiles/exposure_device.json
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from yuki_amd import core as yk  # noqa: E402
from yuki_amd import scenes  # noqa: E402

RESOLUTIONS = ((1920, 1080), (3840, 2160))
FILMS = ("noise", "rendered", "constant", "half_black")
SEED = 0x73B9642E74AC471C
HIST, FINAL, PARTIAL, MM_FINAL, TM_METERED, TM_PLAIN = "k_meter_hist", "k_meter_final", "k_min_max_partial", "k_min_max_final", "k_tone_map<true>", "k_tone_map<false>"


def make_films(ctx, res, scene_name):
    w, h = res
    rng = np.random.default_rng(20261020)
    noise = np.exp2(rng.uniform(-10.0, 10.0, size=(h, w, 3))).astype(np.float32)
    sd = scenes.by_name(scene_name)
    fs = yk.FilmSettings(res=res, tile_dim=16)
    sc = yk.Scene(ctx, sd)
    tiles = yk.film_tiles(fs)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=5)))
    rendered = yk.update_tiles(tiles, it.render_tiles(sc, yk.Camera(sd.camera, fs), yk.SamplerType.Uniform(1, SEED), tiles)[0], res)
    sc.close()
    half = noise.copy()
    half[: h // 2] = 0.0
    return dict(noise=noise, rendered=rendered, constant=np.full((h, w, 3), 0.18, np.float32), half_black=half)


def variants(ctx, stream, d_film, d_out, d_state, res):
    """label -> (the call, the kernels one call launches, in order)."""
    heat = yk.ToneMapType.Heatmap(yk.HeatmapParams(None, yk.HeatmapChannel.Luminance))
    filmic = yk.ToneMapType.default()
    st = stream.cuda_stream

    def meter(combine):
        def call():
            ctx.set_option("exposure_wave_combine", combine)
            ctx.meter_exposure_device(d_film.data_ptr(), res, 16, None, None, d_state.data_ptr(), d_state.data_ptr(), stream=st)

        return call

    return {
        "meter_combine_1": (meter(1), (HIST, FINAL)),
        "min_max_heatmap": (lambda: ctx.tone_map_device(d_film.data_ptr(), res, 16, heat, None, d_out.data_ptr(), stream=st), (PARTIAL, MM_FINAL, TM_PLAIN)),
        "meter_combine_0": (meter(0), (HIST, FINAL)),
        "tone_map_metered": (lambda: ctx.tone_map_device(d_film.data_ptr(), res, 16, filmic, None, d_out.data_ptr(), stream=st, exposure_state=d_state.data_ptr()), (TM_METERED,)),
        "tone_map_plain": (lambda: ctx.tone_map_device(d_film.data_ptr(), res, 16, filmic, None, d_out.data_ptr(), stream=st), (TM_PLAIN,)),
    }


def sequence(a):
    """(resolution, film, label, timed) in the order both runs make the calls: per film, a warm-up of every variant, then the
    variants alternating."""
    for res in RESOLUTIONS:
        for film in FILMS:
            for label in ("meter_combine_1", "min_max_heatmap", "meter_combine_0", "tone_map_metered", "tone_map_plain"):
                yield res, film, label, False
            for _ in range(a.rounds):
                for label in ("meter_combine_1", "min_max_heatmap", "meter_combine_0", "tone_map_metered", "tone_map_plain"):
                    yield res, film, label, True


def run(a, film_dir, with_events):
    """Makes the calls of sequence(); with events, returns {(res, film, label): [us per call]}."""
    ctx = yk.Context(0)
    stream = torch.cuda.Stream()
    times, cur, bufs = {}, None, None
    for res, film, label, timed in sequence(a):
        if cur != (res, film):
            host = np.load(os.path.join(film_dir, f"{film}_{res[0]}x{res[1]}.npy"))
            d_film = torch.from_numpy(host.reshape(-1)).to("cuda:0")
            bufs = variants(ctx, stream, d_film, torch.zeros_like(d_film), torch.zeros(8, dtype=torch.int32, device="cuda:0"), res)
            cur = (res, film)
            torch.cuda.synchronize()
        call, _ = bufs[label]
        n = a.launches if timed else a.warmup
        if not (with_events and timed):
            for _ in range(n):
                call()
            stream.synchronize()
            continue
        events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for e0, e1 in events:
            e0.record(stream)
            call()
            e1.record(stream)
        stream.synchronize()
        times.setdefault((res, film, label), []).extend(e0.elapsed_time(e1) * 1e3 for e0, e1 in events)
    ctx.set_option("exposure_wave_combine", 1)
    ctx.close()
    return times


def summary(us):
    return dict(n=len(us), min_us=round(min(us), 2), median_us=round(statistics.median(us), 2), max_us=round(max(us), 2))


def kernel_times(a, film_dir, trace_dir):
    """The child run under rocprofv3, and its kernel trace matched to sequence(): {(res, film, label, kernel): [us]}."""
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "-o", "run", "--", sys.executable, os.path.abspath(__file__), "--child", film_dir,
           "--warmup", str(a.warmup), "--launches", str(a.launches), "--rounds", str(a.rounds)]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.trace_timeout)
    if done.returncode != 0:
        raise RuntimeError(f"rocprofv3 run failed ({done.returncode}): {done.stdout[-400:]}")
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise RuntimeError(f"expected one kernel trace, found {files}")
    rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(files[0]))))
    mangled = {TM_METERED: "k_tone_mapILb1E", TM_PLAIN: "k_tone_mapILb0E"}  # a trace that keeps the symbols as they are
    queues = {k: [(e - s) * 1e-3 for s, e, name in rows if k in name or mangled.get(k, k) in name] for k in (HIST, FINAL, PARTIAL, MM_FINAL, TM_METERED, TM_PLAIN)}
    launched = {"meter_combine_1": (HIST, FINAL), "min_max_heatmap": (PARTIAL, MM_FINAL, TM_PLAIN), "meter_combine_0": (HIST, FINAL), "tone_map_metered": (TM_METERED,), "tone_map_plain": (TM_PLAIN,)}
    pos = {k: 0 for k in queues}
    out = {}
    for res, film, label, timed in sequence(a):
        n = a.launches if timed else a.warmup
        for k in launched[label]:
            taken = queues[k][pos[k] : pos[k] + n]
            pos[k] += n
            if len(taken) != n:
                raise RuntimeError(f"the trace has fewer {k} dispatches than the sequence")
            if timed:
                out.setdefault((res, film, label, k), []).extend(taken)
    for k in queues:
        if pos[k] != len(queues[k]):
            raise RuntimeError(f"the trace has {len(queues[k])} {k} dispatches, the sequence {pos[k]}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cfg3")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-timeout", type=int, default=420)
    ap.add_argument("--child", default="", help="(internal) make the calls on the films of this directory and exit: the run rocprofv3 traces")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        run(a, a.child, with_events=False)
        return
    with tempfile.TemporaryDirectory() as tmp:
        ctx = yk.Context(0)
        for res in RESOLUTIONS:
            for name, film in make_films(ctx, res, a.scene).items():
                np.save(os.path.join(tmp, f"{name}_{res[0]}x{res[1]}.npy"), film)
        ctx.close()
        print("films made", flush=True)
        calls = run(a, tmp, with_events=True)
        print("calls timed; tracing the child run", flush=True)
        try:
            kernels, trace_note = kernel_times(a, tmp, os.path.join(tmp, "trace")), None
        except (RuntimeError, OSError, subprocess.TimeoutExpired, KeyError) as e:
            kernels, trace_note = {}, f"not measured: {e}"
    result = dict(tool="tools/exposure_bench.py", timing="calls: device events around each call; kernels: rocprofv3 --kernel-trace --stats of a child run of the same sequence",
                  scene=a.scene, warmup=a.warmup, launches=a.launches, rounds=a.rounds, kernel_trace=trace_note or "measured", films={})
    for res in RESOLUTIONS:
        key = f"{res[0]}x{res[1]}"
        result["films"][key] = {}
        for film in FILMS:
            entry = dict(calls={label: summary(calls[(res, film, label)]) for label in ("meter_combine_1", "min_max_heatmap", "meter_combine_0", "tone_map_metered", "tone_map_plain")})
            entry["kernels"] = {f"{label}/{k}": summary(v) for (r, f, label, k), v in kernels.items() if r == res and f == film} or "not measured"
            result["films"][key][film] = entry
            print(key, film, json.dumps(entry), flush=True)
    if kernels:
        k4 = RESOLUTIONS[1]
        med = lambda film, label, k: statistics.median(kernels[(k4, film, label, k)])
        plain, metered = kernels[(k4, "rendered", "tone_map_plain", TM_PLAIN)], kernels[(k4, "rendered", "tone_map_metered", TM_METERED)]
        result["done_when"] = dict(
            hist_over_min_max_partial_4k={f: round(med(f, "meter_combine_1", HIST) / med(f, "min_max_heatmap", PARTIAL), 3) for f in ("noise", "rendered")},
            hist_within_2x_of_min_max_partial_4k=all(med(f, "meter_combine_1", HIST) <= 2 * med(f, "min_max_heatmap", PARTIAL) for f in ("noise", "rendered")),
            constant_over_noise_4k={"combine_0": round(med("constant", "meter_combine_0", HIST) / med("noise", "meter_combine_0", HIST), 3), "combine_1": round(med("constant", "meter_combine_1", HIST) / med("noise", "meter_combine_1", HIST), 3)},
            tone_map_ranges_overlap_4k=bool(min(metered) <= max(plain) and min(plain) <= max(metered)),
        )
        print("done_when", json.dumps(result["done_when"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
