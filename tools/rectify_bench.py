#!/usr/bin/env python3
"""Device time of history rectification (yk_history_rectify_device, k_rectify) on cfg3 at 1920 x 1080, every film resident
on the device and cache-warm.

The parent renders two 4-spp films of cfg3 and the guides, blends the first into a history and moments (n = 4) and saves
them; the second film is the current frame.  Then this script runs again as a fresh child process under
`rocprofv3 --kernel-trace --stats`, once per build: the library as built (one k_rectify instance per radius, FilmTile<1..3>,
loops unrolled) and a timing build with one instance under a halo of 3 and a run-time radius
(tools/build_variant.sh one -DYK_RECTIFY_ONE_INSTANCE).  A child rectifies at every radius, with and without moments, and —
beside it, in the same run — blends the film (k_record_blend) and takes the all-spatial variance (k_variance without
moments).  Kernel times come from the trace; the outputs of the two builds are compared by checksum.  k_rectify's time is
reported over its bytes at the 8 TB/s peak.

    tools/build_variant.sh one -DYK_RECTIFY_ONE_INSTANCE
    python tools/rectify_bench.py --out profiles/rectify_device.json
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
RADII = (1, 2, 3)
HBM_PEAK = 8.0e12  # bytes / s, the specified peak
SEED = 0x73B9642E74AC471C
SPP = 4


def summary(us):
    return dict(n=len(us), min_us=round(min(us), 2), median_us=round(statistics.median(us), 2), max_us=round(max(us), 2))


def bound_bytes(with_moments):
    """What one rectification has to move at least: the film read once, every record read once and written once."""
    return RES[0] * RES[1] * (12 + (64 if with_moments else 32))


# ------------------------------------------------------------------ the child: the kernels alone, on saved records
def child(a):
    d = a.child
    ctx = yk.Context(0)
    stream = torch.cuda.Stream()
    cs = stream.cuda_stream
    dev = lambda name: torch.from_numpy(np.load(os.path.join(d, name + ".npy")).view(np.float32).reshape(-1)).to("cuda:0")  # noqa: E731
    film, hist, mom, guides = dev("film"), dev("history"), dev("moments"), dev("guides")
    n = RES[0] * RES[1]
    out_h, out_m = torch.zeros(4 * n, dtype=torch.float32, device="cuda:0"), torch.zeros(4 * n, dtype=torch.float32, device="cuda:0")
    rgb, var = torch.zeros(3 * n, dtype=torch.float32, device="cuda:0"), torch.zeros(n, dtype=torch.float32, device="cuda:0")
    samples = np.full((-(-RES[0] // 16)) * (-(-RES[1] // 16)), SPP, np.uint32)
    res = {}
    torch.cuda.synchronize()

    def repeat(call):
        for _ in range(a.warmup + a.launches):
            call()
        stream.synchronize()

    for radius in RADII:
        p = yk.RectifyParams(radius=radius, gamma=a.gamma)
        for with_m in (False, True):
            repeat(lambda: ctx.rectify_history_device(film.data_ptr(), RES, p, 16, samples, hist.data_ptr(), out_h.data_ptr(), stream=cs, moments=mom.data_ptr() if with_m else None,
                                                      out_moments=out_m.data_ptr() if with_m else None))
            res[f"r{radius}{'_moments' if with_m else ''}_checksum"] = int(out_h.view(torch.int32).to(torch.int64).sum().item()) + (int(out_m.view(torch.int32).to(torch.int64).sum().item()) if with_m else 0)
        res[f"r{radius}_clipped"] = float((out_h.view(-1, 4)[:, 3] != hist.view(-1, 4)[:, 3]).float().mean().item())
    tp = yk.TemporalParams(max_history=64.0)
    repeat(lambda: ctx.blend_history_device(film.data_ptr(), RES, tp, 16, samples, hist.data_ptr(), out_h.data_ptr(), rgb.data_ptr(), stream=cs))
    vp = yk.VarianceParams(sigma_plane=a.sigma_plane)
    repeat(lambda: ctx.variance_device(None, film.data_ptr(), guides.data_ptr(), RES, vp, 16, samples, var.data_ptr(), stream=cs))
    ctx.close()
    print("CHILD " + json.dumps(res), flush=True)


class ChildFailed(Exception):
    """A GPU child process ended with a non-zero status.  Never caught: nothing more is started on the device after it."""


def traced_child(a, d, lib, trace_dir):
    """A fresh process on the saved records under rocprofv3: (what the child printed, {kernel: [us per dispatch after the
    warm-up]}).  A child that fails or runs past its time limit ends the whole script."""
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "-o", "run", "--", sys.executable, os.path.abspath(__file__), "--child", d, "--warmup", str(a.warmup),
           "--launches", str(a.launches), "--gamma", str(a.gamma), "--sigma-plane", str(a.sigma_plane)]
    env = dict(os.environ)
    if lib:
        env["YK_LIB_PATH"] = lib
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout, env=env)
    if done.returncode != 0:
        raise ChildFailed(f"child failed ({done.returncode}): {done.stdout[-600:]}")
    printed = json.loads([ln for ln in done.stdout.splitlines() if ln.startswith("CHILD ")][-1][6:])
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise RuntimeError(f"expected one kernel trace, found {files}")
    rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(files[0]))))
    per = a.warmup + a.launches
    rect = [(e - s) * 1e-3 for s, e, name in rows if "k_rectify" in name]
    if len(rect) != per * 2 * len(RADII):
        raise RuntimeError(f"the trace has {len(rect)} k_rectify dispatches, the run {per * 2 * len(RADII)}")
    out = {}
    k = 0
    for radius in RADII:
        for with_m in (False, True):
            out[f"k_rectify_r{radius}{'_moments' if with_m else ''}"] = rect[k * per + a.warmup : (k + 1) * per]
            k += 1
    for what in ("k_record_blend", "k_variance"):
        t = [(e - s) * 1e-3 for s, e, name in rows if what in name]
        if len(t) != per:
            raise RuntimeError(f"the trace has {len(t)} {what} dispatches, the run {per}")
        out[what] = t[a.warmup :]
    return printed, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cfg3")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--gamma", type=float, default=yk.RectifyParams().gamma)
    ap.add_argument("--sigma-plane", type=float, default=0.0)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--one-lib", default=os.path.join(ROOT, "yuki_amd", "libyuki_hip_one.so"))
    ap.add_argument("--child", default="", help="(internal) run the kernels on the records saved in this directory and exit")
    ap.add_argument("--bench-this", nargs="*", default=[], help="result lines of separate `bench.py` runs on this build (files), recorded beside the measurements")
    ap.add_argument("--bench-parent", nargs="*", default=[], help="the same of the parent commit's build, run alternating with them")
    ap.add_argument("--bench-cmd", default="python bench.py --gpus 1 --steps 10 --warmup 3")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    result = dict(tool="tools/rectify_bench.py", scene=a.scene, film=list(RES), spp=SPP, gamma=a.gamma, warmup=a.warmup, launches=a.launches,
                  timing="rocprofv3 --kernel-trace --stats of one child run per build; films resident, every call repeated on the same buffers")
    with tempfile.TemporaryDirectory() as tmp:
        ctx = yk.Context(0)
        sd = scenes.by_name(a.scene)
        sc = yk.Scene(ctx, sd)
        a.sigma_plane = yk.VarianceParams.for_scene(sc).sigma_plane
        fs = yk.FilmSettings(res=RES, tile_dim=16)
        cam = yk.Camera(sd.camera, fs)
        tiles = yk.film_tiles(fs)
        it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=8)))
        render = lambda seed: yk.update_tiles(tiles, it.render_tiles(sc, cam, yk.SamplerType.Uniform(SPP, seed), tiles)[0], fs.res)  # noqa: E731
        before, now = render(SEED), render(SEED + 977)
        guides = yk.render_guides(ctx, sc, cam, fs)
        sc.close()
        ctx.close()
        torch.cuda.empty_cache()
        tp = yk.TemporalParams(max_history=64.0)
        samples = np.full((-(-RES[0] // 16)) * (-(-RES[1] // 16)), SPP, np.uint32)
        _, hist = yk.blend_history(before * np.float32(SPP), tp, samples=samples)
        mom = yk.blend_moments(before * np.float32(SPP), tp, samples=samples)
        for name, arr in (("film", now * np.float32(SPP)), ("history", hist), ("moments", mom), ("guides", guides)):
            np.save(os.path.join(tmp, name + ".npy"), np.ascontiguousarray(arr).view(np.float32))
        builds = {"per_radius": None}
        if os.path.exists(a.one_lib):
            builds["one_instance"] = a.one_lib
        else:
            result["one_instance"] = f"not measured: {os.path.relpath(a.one_lib, ROOT)} is not built (tools/build_variant.sh one -DYK_RECTIFY_ONE_INSTANCE)"
        printed, times = {}, {}
        for b, lib in builds.items():  # a child that fails or hangs ends the script here
            printed[b], times[b] = traced_child(a, tmp, lib, os.path.join(tmp, "trace_" + b))
    result["kernels_us"] = {b: {k: summary(v) for k, v in t.items()} for b, t in times.items()}
    result["clipped_share"] = {k: round(v, 4) for k, v in printed["per_radius"].items() if k.endswith("_clipped")}
    if "one_instance" in printed:
        result["outputs_identical"] = all(printed["per_radius"][k] == printed["one_instance"][k] for k in printed["per_radius"] if k.endswith("_checksum"))
    result["bound"] = {}
    for with_m in (False, True):
        b = bound_bytes(with_m)
        entry = dict(bytes=b, hbm_peak_bytes_per_s=HBM_PEAK, bound_us=round(b / HBM_PEAK * 1e6, 2))
        for radius in RADII:
            med = statistics.median(times["per_radius"][f"k_rectify_r{radius}{'_moments' if with_m else ''}"])
            entry[f"r{radius}"] = dict(kernel_us=round(med, 2), time_over_bound=round(med / (b / HBM_PEAK * 1e6), 2), gbytes_per_s=round(b / med * 1e-3, 1))
        result["bound"]["with_moments" if with_m else "history_only"] = entry
    if a.bench_this or a.bench_parent:
        value = lambda path: round(json.load(open(path))["value"], 1)  # noqa: E731
        result["bench_py"] = dict(cmd=a.bench_cmd, unit="Mray/s", note="not measured by this tool: the result lines of separate bench.py runs, this build and the parent commit's build alternating, handed in with --bench-this / --bench-parent",
                                  this_build=[value(f) for f in a.bench_this], parent_build=[value(f) for f in a.bench_parent])
    print("kernels (us):", {b: {k: v["median_us"] for k, v in t.items()} for b, t in result["kernels_us"].items()}, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
