#!/usr/bin/env python3
"""Device time of one yk_present_device launch (k_present), per case, from device events.

A case is film -> window in a frame format: `1080p_1080p_rgba8`, `1080p_2160p_rgba8`, `1080p_2160p_rgb32f` (encode 2, the
sRGB back buffer).  Per case: `--warmup` launches, then `--launches` launches, each between its own pair of events on the
caller's stream; recorded are the times of every launch, the bytes the pass must move (the film read once plus the frame
written once) and the rate that gives against the 6.29 TB/s copy ceiling.  The frame of the last launch is compared
with the host instance.  `--out` merges the cases it ran into an existing file, so that each case can be a process of
its own:

    python tools/present_bench.py --cases 1080p_1080p_rgba8 --out profiles/present_device.json
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

COPY_CEILING_GBPS = 6290.0  # the measured copy ceiling of the MI355X the project compares with
SIZES = {"1080p": (1920, 1080), "2160p": (3840, 2160)}
CASES = ("1080p_1080p_rgba8", "1080p_2160p_rgba8", "1080p_2160p_rgb32f")


def run_case(ctx, name, warmup, launches):
    film_name, window_name, fmt = name.split("_")
    res, window = SIZES[film_name], SIZES[window_name]
    film = np.random.default_rng(31).random((res[1], res[0], 3), dtype=np.float32)
    d_film = torch.from_numpy(film.reshape(-1)).to("cuda:0")
    words = window[0] * window[1] * (1 if fmt == "rgba8" else 3)
    d_frame = torch.zeros(words, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(warmup):
        ctx.present_device(d_film.data_ptr(), res, window, 2, fmt, d_frame.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in events:
        a.record(stream)
        ctx.present_device(d_film.data_ptr(), res, window, 2, fmt, d_frame.data_ptr(), stream=stream.cuda_stream)
        b.record(stream)
    stream.synchronize()
    us = [a.elapsed_time(b) * 1e3 for a, b in events]
    want = yk.present(film, window, 2, fmt)
    got = d_frame.cpu().numpy()
    got = got.view(np.uint8).reshape(want.shape) if fmt == "rgba8" else got.view(np.float32).reshape(want.shape)
    equal = bool(np.array_equal(got.view(np.uint8), want.view(np.uint8)))
    moved = res[0] * res[1] * 12 + words * 4
    med = statistics.median(us)
    rec = dict(film=list(res), window=list(window), format=fmt, encode=2, warmup=warmup, launches=launches, launch_us=[round(t, 2) for t in us],
               min_us=round(min(us), 2), median_us=round(med, 2), max_us=round(max(us), 2), bytes_moved=moved,
               gbps_at_median=round(moved / med * 1e-3, 1), share_of_copy_ceiling=round(moved / med * 1e-3 / COPY_CEILING_GBPS, 3),
               equals_host_instance=equal)
    print(name, json.dumps({k: v for k, v in rec.items() if k != "launch_us"}), flush=True)
    assert equal, "the device frame differs from the host instance"
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    result = dict(tool="tools/present_bench.py", timing="device events around each launch", copy_ceiling_gbps=COPY_CEILING_GBPS, cases={})
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            result["cases"] = json.load(f).get("cases", {})
    ctx = yk.Context(0)
    for name in a.cases.split(","):
        result["cases"][name] = run_case(ctx, name, a.warmup, a.launches)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
