#!/usr/bin/env python3
"""Device time of the guide pass through glass (yk_render_guides_through_device, k_guides_step) at 1920 x 1080, every
buffer resident on the device.

Per scene (cfg3: 10 % glass; cfg5, the metal / glass mix: 50 % glass):
  - Calls: yk_render_guides_ids_device (the first-hit pass, untouched by this feature) and yk_render_guides_through_device at
    max_through 0, 1, 4 and 8, each timed with a pair of device events on the caller's stream, the variants interleaved
    round by round in the same run so that they see the same machine.
  - Rays: how many rays each pass traced, from the `through` record of a max_through = 8 call read back AFTER the call (a
    pixel that crossed t interfaces had a ray in passes 0 .. t); the library itself reads nothing back.
  - Kernels: a run of its own — this script again as a fresh child process under `rocprofv3 --kernel-trace --stats`, making
    the same calls; k_guides_step and the closest-hit trace are reported per pass of the max_through = 8 call.

    python tools/guides_through_device.py --out profiles/guides_through_device.json
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
VARIANTS = ("ids", 0, 1, 4, 8)  # "ids": yk_render_guides_ids_device; a number: yk_render_guides_through_device at that max_through


def summary(v, unit):
    return {"n": len(v), "min_" + unit: round(min(v), 2), "median_" + unit: round(statistics.median(v), 2), "max_" + unit: round(max(v), 2)}


class Job:
    """Scene, camera and the three device buffers of one scene."""

    def __init__(self, name):
        self.ctx = yk.Context(0)
        sd = scenes.by_name(name)
        self.sc = yk.Scene(self.ctx, sd)
        self.fs = yk.FilmSettings(res=RES, tile_dim=16)
        self.cam = yk.Camera(sd.camera, self.fs)
        n = RES[0] * RES[1]
        self.guides = torch.zeros(8 * n, dtype=torch.float32, device="cuda:0")
        self.ids = torch.zeros(4 * n, dtype=torch.int32, device="cuda:0")
        self.through = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        self.stream = torch.cuda.Stream()
        torch.cuda.synchronize()

    def call(self, variant):
        cs = self.stream.cuda_stream
        if variant == "ids":
            self.ctx.render_guides_ids_device(self.sc, self.cam, RES, self.guides.data_ptr(), self.ids.data_ptr(), stream=cs)
        else:
            self.ctx.render_guides_through_device(self.sc, self.cam, RES, self.guides.data_ptr(), self.ids.data_ptr(), self.through.data_ptr(), max_through=variant, stream=cs)

    def close(self):
        self.sc.close()
        self.ctx.close()


def time_calls(job, warmup, rounds):
    """{variant: [ms]}: one event pair around every call, the variants interleaved."""
    ms = {v: [] for v in VARIANTS}
    for r in range(warmup + rounds):
        for v in VARIANTS:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(job.stream)
            job.call(v)
            b.record(job.stream)
            job.stream.synchronize()
            if r >= warmup:
                ms[v].append(a.elapsed_time(b))
    return ms


def rays_per_pass(job):
    job.call(8)
    job.stream.synchronize()
    t = job.through.cpu().numpy()
    hit = job.guides.view(-1, 8)[:, 3].cpu().numpy() != 0
    return dict(rays=[int((t >= k).sum()) for k in range(9)], pixels_by_interfaces=np.bincount(t, minlength=9).tolist(), glass_first_hits=int((t >= 1).sum()),
                hit_behind_glass=int(((t >= 1) & hit).sum()))


# ------------------------------------------------------------------ the child: the same calls, traced
def child(a):
    job = Job(a.child)
    for v in VARIANTS:
        for _ in range(a.warmup + a.launches):
            job.call(v)
        job.stream.synchronize()
    job.close()
    print("CHILD done", flush=True)


def traced_child(a, name, trace_dir):
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "-o", "run", "--", sys.executable, os.path.abspath(__file__), "--child", name, "--warmup", str(a.warmup),
           "--launches", str(a.launches)]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout)
    if done.returncode != 0:  # never caught: nothing more is started on the device after a child that failed
        raise RuntimeError(f"child failed ({done.returncode}): {done.stdout[-600:]}")
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise RuntimeError(f"expected one kernel trace, found {files}")
    rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(files[0]))))
    per = a.warmup + a.launches
    passes = {"ids": 1, 0: 1, 1: 2, 4: 5, 8: 9}
    out = {}
    is_kernel = {"k_guides_step": lambda k: "k_guides_step" in k, "k_trace_closest": lambda k: "k_trace_closest" in k, "k_guides": lambda k: "k_guides" in k and "k_guides_step" not in k}
    for what, calls_with in (("k_guides_step", [v for v in VARIANTS if v != "ids"]), ("k_trace_closest", list(VARIANTS)), ("k_guides", ["ids"])):
        t = [(e - s) * 1e-3 for s, e, kname in rows if is_kernel[what](kname)]
        want = per * sum(passes[v] for v in calls_with)
        if len(t) != want:  # said, not guessed around: the per-pass split below needs the exact sequence
            out[what + "/unmatched"] = f"the trace has {len(t)} dispatches, the run {want}; total {round(sum(t), 1)} us"
            continue
        at = 0
        for v in calls_with:
            k = passes[v]
            block = t[at : at + per * k]
            at += per * k
            for p in range(k):
                out[f"{what}/{v}/pass{p}"] = summary([block[c * k + p] for c in range(a.warmup, per)], "us")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="*", default=["cfg3", "cfg5"])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=15)
    ap.add_argument("--child-timeout", type=int, default=280)
    ap.add_argument("--child", default="", help="(internal) make the calls on this scene and exit: the run rocprofv3 traces")
    ap.add_argument("--no-trace", action="store_true", help="calls and ray counts only")
    ap.add_argument("--bench-this", nargs="*", default=[], help="result lines of separate `bench.py` runs on this build (files), recorded beside the measurements")
    ap.add_argument("--bench-parent", nargs="*", default=[], help="the same of the parent commit's build, run alternating with them")
    ap.add_argument("--bench-cmd", default="python bench.py --gpus 1 --steps 10 --warmup 3")
    ap.add_argument("--earlier", default="", help="the output of this tool on an earlier build of k_guides_step: its k_guides_step times and call times are recorded beside this run's")
    ap.add_argument("--earlier-name", default="per_wave_atomic")
    ap.add_argument("--earlier-note", default="k_guides_step with one global atomic per wave instead of one per block; an earlier run on the same machine type, not interleaved with this one")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    result = dict(tool="tools/guides_through_device.py", film=list(RES), warmup=a.warmup, launches=a.launches,
                  timing="calls: device events around each call on the caller's stream, variants interleaved; kernels: rocprofv3 --kernel-trace --stats of a fresh child run of the same calls",
                  variants={"ids": "yk_render_guides_ids_device", "0/1/4/8": "yk_render_guides_through_device at that max_through"}, scenes={})
    for name in a.scenes:
        job = Job(name)
        entry = dict(rays=rays_per_pass(job))
        ms = time_calls(job, a.warmup, a.launches)
        entry["calls_ms"] = {str(v): summary(t, "ms") for v, t in ms.items()}
        job.close()
        torch.cuda.empty_cache()
        print(name, "calls (median ms):", {str(v): round(statistics.median(t), 3) for v, t in ms.items()}, "rays:", entry["rays"]["rays"], flush=True)
        if not a.no_trace:
            with tempfile.TemporaryDirectory() as tmp:
                entry["kernels_us"] = traced_child(a, name, os.path.join(tmp, "trace"))
            print(name, "k_guides_step of max_through 8 (median us):", [entry["kernels_us"].get(f"k_guides_step/8/pass{p}", {}).get("median_us") for p in range(9)], flush=True)
        result["scenes"][name] = entry
    if a.bench_this or a.bench_parent:
        value = lambda path: round(json.load(open(path))["value"], 1)  # noqa: E731
        result["bench_py"] = dict(cmd=a.bench_cmd, note="not measured by this tool: the result lines of separate bench.py runs, this build and the parent commit's build alternating, handed in with --bench-this / --bench-parent",
                                  this_build=[value(f) for f in a.bench_this], parent_build=[value(f) for f in a.bench_parent])
    if a.earlier:
        old = json.load(open(a.earlier))
        result[a.earlier_name] = dict(note=a.earlier_note, scenes={name: dict(calls_ms=e["calls_ms"], kernels_us={k: v for k, v in e.get("kernels_us", {}).items() if k.startswith("k_guides_step")})
                                                                  for name, e in old["scenes"].items()})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
