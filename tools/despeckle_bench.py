#!/usr/bin/env python3
"""Device time of the despeckle pass (yk_despeckle_device, k_despeckle) on cfg3 at 1920 x 1080, every film resident on the
device and cache-warm.

The parent renders two 4-spp films of cfg3, blends the first into a history (n = 4) and saves them; the second film is the
current frame.  Then this script runs again as a fresh child process under `rocprofv3 --kernel-trace --stats` (no counters
in the same run).  The child despeckles at radius 1 and 2 — without mask and counts, with both, and with each
alone — and, beside it in the same run as yardsticks, rectifies the history at radius 1 and 2 (k_rectify, which stages the same tile and walks the window
twice) and blends the film (k_record_blend, the streaming floor of a film pass).  Kernel times come from the trace: the
median of the dispatches after the warm-up.  k_despeckle's time is reported over its bytes — 12 in and 12 out a pixel — at
the 8 TB/s peak.

    python tools/despeckle_bench.py --out profiles/despeckle_device.json
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

RES = (1920, 1080)
RADII = (1, 2)
HBM_PEAK = 8.0e12  # bytes / s, the specified peak
SEED = 0x73B9642E74AC471C
SPP = 4
BOUND_BYTES = RES[0] * RES[1] * 24  # the film read once and written once


def summary(us):
    return dict(n=len(us), min_us=round(min(us), 2), median_us=round(statistics.median(us), 2), max_us=round(max(us), 2))


def params(radius):
    d = yk.DespeckleParams()
    return yk.DespeckleParams(radius=radius, rank=d.rank, gain=d.gain)


# ------------------------------------------------------------------ the child: the kernels alone, on saved films
def child(a):
    d = a.child
    ctx = yk.Context(0)
    stream = torch.cuda.Stream()
    cs = stream.cuda_stream
    dev = lambda name: torch.from_numpy(np.load(os.path.join(d, name + ".npy")).view(np.float32).reshape(-1)).to("cuda:0")  # noqa: E731
    film, hist = dev("film"), dev("history")
    n = RES[0] * RES[1]
    out, out_h, rgb = torch.zeros(3 * n, dtype=torch.float32, device="cuda:0"), torch.zeros(4 * n, dtype=torch.float32, device="cuda:0"), torch.zeros(3 * n, dtype=torch.float32, device="cuda:0")
    mask, counts = torch.zeros(n, dtype=torch.uint8, device="cuda:0"), torch.zeros(2, dtype=torch.int32, device="cuda:0")
    samples = np.full((-(-RES[0] // 16)) * (-(-RES[1] // 16)), SPP, np.uint32)
    res = {}
    torch.cuda.synchronize()

    def repeat(call):
        for _ in range(a.warmup + a.launches):
            call()
        stream.synchronize()

    for radius in RADII:
        p = params(radius)
        repeat(lambda: ctx.despeckle_device(film, RES, p, 16, samples, out, stream=cs))
        bare = int(out.view(torch.int32).to(torch.int64).sum().item())
        repeat(lambda: ctx.despeckle_device(film, RES, p, 16, samples, out, stream=cs, mask=mask, counts=counts))
        res[f"r{radius}_same_film_with_and_without_mask"] = bare == int(out.view(torch.int32).to(torch.int64).sum().item())
        res[f"r{radius}_clamped"] = int(counts[0].item())
        res[f"r{radius}_mask_agrees"] = int((mask == 1).sum().item()) == int(counts[0].item())
        repeat(lambda: ctx.despeckle_device(film, RES, p, 16, samples, out, stream=cs, mask=mask))
        repeat(lambda: ctx.despeckle_device(film, RES, p, 16, samples, out, stream=cs, counts=counts))
    for radius in RADII:
        rp = yk.RectifyParams(radius=radius)
        repeat(lambda: ctx.rectify_history_device(film.data_ptr(), RES, rp, 16, samples, hist.data_ptr(), out_h.data_ptr(), stream=cs))
    tp = yk.TemporalParams(max_history=64.0)
    repeat(lambda: ctx.blend_history_device(film.data_ptr(), RES, tp, 16, samples, hist.data_ptr(), out_h.data_ptr(), rgb.data_ptr(), stream=cs))
    ctx.close()
    print("CHILD " + json.dumps(res), flush=True)


class ChildFailed(Exception):
    """A GPU child process ended with a non-zero status.  Never caught: nothing more is started on the device after it."""


def traced_child(a, d, trace_dir):
    """A fresh process on the saved films under rocprofv3: (what the child printed, {kernel: [us per dispatch after the
    warm-up]}).  A child that fails or runs past its time limit ends the whole script."""
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "-o", "run", "--", sys.executable, os.path.abspath(__file__), "--child", d, "--warmup", str(a.warmup),
           "--launches", str(a.launches)]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout)
    if done.returncode != 0:
        raise ChildFailed(f"child failed ({done.returncode}): {done.stdout[-600:]}")
    printed = json.loads([ln for ln in done.stdout.splitlines() if ln.startswith("CHILD ")][-1][6:])
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise RuntimeError(f"expected one kernel trace, found {files}")
    rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(files[0]))))
    per = a.warmup + a.launches
    out = {}
    for what, variants in (("k_despeckle", [f"r{r}{m}" for r in RADII for m in ("", "_mask_counts", "_mask", "_counts")]), ("k_rectify", [f"r{r}" for r in RADII]), ("k_record_blend", [""])):
        t = [(e - s) * 1e-3 for s, e, name in rows if what in name]
        if len(t) != per * len(variants):
            raise RuntimeError(f"the trace has {len(t)} {what} dispatches, the run {per * len(variants)}")
        for k, v in enumerate(variants):
            out[what + ("_" + v if v else "")] = t[k * per + a.warmup : (k + 1) * per]
    return printed, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cfg3")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--child", default="", help="(internal) run the kernels on the films saved in this directory and exit")
    ap.add_argument("--bench-this", nargs="*", default=[], help="result lines of separate `bench.py` runs on this build (files), recorded beside the measurements")
    ap.add_argument("--bench-parent", nargs="*", default=[], help="the same of the parent commit's build, run alternating with them")
    ap.add_argument("--bench-cmd", default="python bench.py --gpus 1 --steps 10 --warmup 3")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    d = yk.DespeckleParams()
    result = dict(tool="tools/despeckle_bench.py", scene=a.scene, film=list(RES), spp=SPP, rank=d.rank, gain=d.gain, warmup=a.warmup, launches=a.launches,
                  timing="rocprofv3 --kernel-trace --stats of one child run; films resident, every call repeated on the same buffers; medians of the dispatches after the warm-up")
    with tempfile.TemporaryDirectory() as tmp:
        ctx = yk.Context(0)
        sd = scenes.by_name(a.scene)
        sc = yk.Scene(ctx, sd)
        fs = yk.FilmSettings(res=RES, tile_dim=16)
        cam = yk.Camera(sd.camera, fs)
        tiles = yk.film_tiles(fs)
        it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=8)))
        render = lambda seed: yk.update_tiles(tiles, it.render_tiles(sc, cam, yk.SamplerType.Uniform(SPP, seed), tiles)[0], fs.res)  # noqa: E731
        before, now = render(SEED), render(SEED + 977)
        sc.close()
        ctx.close()
        torch.cuda.empty_cache()
        samples = np.full((-(-RES[0] // 16)) * (-(-RES[1] // 16)), SPP, np.uint32)
        _, hist = yk.blend_history(before * np.float32(SPP), yk.TemporalParams(max_history=64.0), samples=samples)
        for name, arr in (("film", now * np.float32(SPP)), ("history", hist)):
            np.save(os.path.join(tmp, name + ".npy"), np.ascontiguousarray(arr).view(np.float32))
        printed, times = traced_child(a, tmp, os.path.join(tmp, "trace"))  # a child that fails or hangs ends the script here
    result["kernels_us"] = {k: summary(v) for k, v in times.items()}
    result["child"] = printed
    bound_us = BOUND_BYTES / HBM_PEAK * 1e6
    result["bound"] = dict(bytes=BOUND_BYTES, bytes_per_pixel=24, hbm_peak_bytes_per_s=HBM_PEAK, bound_us=round(bound_us, 2))
    for radius in RADII:
        med = statistics.median(times[f"k_despeckle_r{radius}"])
        rect = statistics.median(times[f"k_rectify_r{radius}"])
        result["bound"][f"r{radius}"] = dict(kernel_us=round(med, 2), time_over_bound=round(med / bound_us, 2), gbytes_per_s=round(BOUND_BYTES / med * 1e-3, 1), over_k_rectify=round(med / rect, 3))
    if a.bench_this or a.bench_parent:
        value = lambda path: round(json.load(open(path))["value"], 1)  # noqa: E731
        result["bench_py"] = dict(cmd=a.bench_cmd, unit="Mray/s", note="not measured by this tool: the result lines of separate bench.py runs, this build and the parent commit's build alternating, handed in with --bench-this / --bench-parent",
                                  this_build=[value(f) for f in a.bench_this], parent_build=[value(f) for f in a.bench_parent])
    print("kernels (us):", {k: v["median_us"] for k, v in result["kernels_us"].items()}, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
