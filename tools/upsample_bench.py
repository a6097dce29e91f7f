#!/usr/bin/env python3
"""Device time of the guided upsample (yk_upsample_device, k_upsample) on cfg3 with a textured ground, full film
1920 x 1080, s = 2 and 4, every film resident on the device.

  - Kernel time: a run of its own — this script again as a fresh child process under `rocprofv3 --kernel-trace --stats` —
    with k_reproject (zero motion) and one k_atrous iteration at 1080p re-measured beside k_upsample in the same run.  The
    kernel's time is reported over the bytes-over-peak bound computed from the shapes.
  - LDS staging against direct loads: the library as built and a timing build whose kernel reads the low window straight
    from global memory (tools/build_variant.sh direct -DYK_UPSAMPLE_DIRECT) alternate as child processes on the same
    films, five runs each, device events around every call; the outputs of the two builds are compared bit for bit.
  - End to end, device events to a final synchronise, the two routes alternating, five each:
      full  4 spp at 1920 x 1080 + guides/ids + albedo + 4-iteration demodulated denoise + tone map;
      low   4 spp at 1/s + low guides + full guides/ids + albedo + mean albedo + low denoise + upsample + tone map.

    tools/build_variant.sh direct -DYK_UPSAMPLE_DIRECT
    python tools/upsample_bench.py --out profiles/upsample_device.json
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

from yuki_amd import abi  # noqa: E402
from yuki_amd import core as yk  # noqa: E402
from yuki_amd import scenes  # noqa: E402

RES = (1920, 1080)
FACTORS = (2, 4)
HBM_PEAK = 8.0e12  # bytes / s, the specified peak
SEED = 0x73B9642E74AC471C


def summary(us):
    return dict(n=len(us), min_us=round(min(us), 2), median_us=round(statistics.median(us), 2), max_us=round(max(us), 2))


def bound_bytes(s, with_albedo=True):
    """What one upsample has to move at least: every full record read once and the RGB written, the low records once."""
    n = RES[0] * RES[1]
    return n * (32 + (16 if with_albedo else 0) + 12) + (n // (s * s)) * (12 + 32 + (16 if with_albedo else 0))


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


# ------------------------------------------------------------------ the child: the kernels alone, on saved records
def child(a):
    """Upsamples the saved films at every factor (and, with --beside, reprojects and runs one à-trous iteration at 1080p);
    prints the event times and a checksum of every output as one JSON line."""
    d = a.child
    meta = json.load(open(os.path.join(d, "meta.json")))
    ctx = yk.Context(0)
    stream = torch.cuda.Stream()
    cs = stream.cuda_stream
    dev = lambda name: torch.from_numpy(np.load(os.path.join(d, name + ".npy")).view(np.float32).reshape(-1)).to("cuda:0")  # noqa: E731
    guides, albedo = dev("guides"), dev("albedo")
    n = RES[0] * RES[1]
    out = torch.zeros(3 * n, dtype=torch.float32, device="cuda:0")
    res = {}
    for s in FACTORS:
        low, lg, la = dev(f"low_s{s}"), dev(f"low_guides_s{s}"), dev(f"low_albedo_s{s}")
        lres = (RES[0] // s, RES[1] // s)
        p = yk.UpsampleParams(s, meta["sigma_normal"], meta["sigma_plane"])
        torch.cuda.synchronize()
        call = lambda: ctx.upsample_device(low.data_ptr(), lg.data_ptr(), lres, guides.data_ptr(), p, 16, None, out.data_ptr(), stream=cs, low_albedo=la.data_ptr(), albedo=albedo.data_ptr())  # noqa: E731
        res[f"s{s}"] = timed(stream, a.launches, a.warmup, call)
        res[f"s{s}_checksum"] = int(out.view(torch.int32).to(torch.int64).sum().item())
    if a.beside:
        fs = yk.FilmSettings(res=RES, tile_dim=16)
        cam = yk.Camera(meta["camera"], fs)
        hist = torch.ones(4 * n, dtype=torch.float32, device="cuda:0")
        rec = torch.zeros(4 * n, dtype=torch.float32, device="cuda:0")
        film = dev("full_film")
        tp = yk.TemporalParams(plane_tolerance=meta["sigma_plane"])
        dp = yk.DenoiseParams(1, 4.0, meta["sigma_normal"], meta["sigma_plane"])
        torch.cuda.synchronize()
        res["reproject"] = timed(stream, a.launches, a.warmup, lambda: ctx.reproject_history_device(hist.data_ptr(), guides.data_ptr(), cam, guides.data_ptr(), RES, tp, rec.data_ptr(), stream=cs))
        res["atrous_one_iteration"] = timed(stream, a.launches, a.warmup, lambda: ctx.denoise_device(film.data_ptr(), guides.data_ptr(), RES, dp, 16, None, out.data_ptr(), stream=cs))
    ctx.close()
    print("CHILD " + json.dumps(res), flush=True)


class ChildFailed(Exception):
    """A GPU child process ended with a non-zero status.  Never caught: nothing more is started on the device after it."""


def run_child(a, d, lib=None, beside=False, trace_dir=None):
    """A fresh process on the saved records.  A child that fails (ChildFailed) or runs past its time limit
    (subprocess.TimeoutExpired) ends the whole script: a fault, an abort or a hang on the device is not followed by
    another process on it."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", d, "--warmup", str(a.warmup), "--launches", str(a.launches)] + (["--beside"] if beside else [])
    if trace_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "-o", "run", "--"] + cmd
    env = dict(os.environ)
    if lib:
        env["YK_LIB_PATH"] = lib
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout, env=env)
    if done.returncode != 0:
        raise ChildFailed(f"child failed ({done.returncode}): {done.stdout[-600:]}")
    line = [ln for ln in done.stdout.splitlines() if ln.startswith("CHILD ")][-1]
    return json.loads(line[6:])


def kernel_times(a, d, trace_dir):
    """The child under rocprofv3: {kernel: [us per dispatch after the warm-up]} from the kernel trace."""
    run_child(a, d, beside=True, trace_dir=trace_dir)
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise RuntimeError(f"expected one kernel trace, found {files}")
    rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(files[0]))))
    out = {}
    ups = [(e - s) * 1e-3 for s, e, name in rows if "k_upsample" in name]
    per = a.warmup + a.launches
    if len(ups) != per * len(FACTORS):
        raise RuntimeError(f"the trace has {len(ups)} k_upsample dispatches, the run {per * len(FACTORS)}")
    for k, s in enumerate(FACTORS):
        out[f"k_upsample_s{s}"] = ups[k * per + a.warmup : (k + 1) * per]
    for key, what in (("k_reproject", "k_reproject"), ("k_atrous", "k_atrous")):
        t = [(e - s) * 1e-3 for s, e, name in rows if what in name]
        if len(t) != per:
            raise RuntimeError(f"the trace has {len(t)} {what} dispatches, the run {per}")
        out[key] = t[a.warmup :]
    return out


# ------------------------------------------------------------------ the parent
class Routes:
    """The two routes to a tone-mapped 1920 x 1080 frame, every buffer made once."""

    def __init__(self, ctx, sd, sc, stream):
        self.ctx, self.sc, self.stream, self.cs = ctx, sc, stream, stream.cuda_stream
        self.it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=8)))
        self.smp = yk.SamplerType.Stratified((2, 2), True, SEED)
        self.fs = yk.FilmSettings(res=RES, tile_dim=16, accumulate=True)
        self.cam = yk.Camera(sd.camera, self.fs)
        self.dp = yk.DenoiseParams.for_scene(sc, iterations=4)
        z = lambda k: torch.zeros(k, dtype=torch.float32, device="cuda:0")  # noqa: E731
        n = RES[0] * RES[1]
        self.guides, self.ids, self.albedo, self.clean, self.full = z(8 * n), z(4 * n), z(4 * n), z(3 * n), z(3 * n)
        self.film = {1: self._film(sd, 1)}
        self.low = {}
        for s in FACTORS:
            f = self._film(sd, s)
            nl = n // (s * s)
            f.update(guides=z(8 * nl), albedo=z(4 * nl), clean=z(3 * nl), up=yk.UpsampleParams.for_scene(sc, s))
            self.low[s] = f

    def _film(self, sd, s):
        fs = yk.subsampled(self.fs, s)
        fs.accumulate = True
        tiles = yk.film_tiles(fs)
        lists = [yk.TileList(self.ctx, tiles, np.full(len(tiles), k, np.uint16)) for k in range(4)]
        return dict(fs=fs, cam=yk.Camera(sd.camera, fs), lists=lists, samples=yk.film_samples(fs, tiles, np.full(len(tiles), 4, np.uint32)), td=yk.film_tile_dim(fs),
                    slab=torch.zeros(lists[0].n_pixels * 3, dtype=torch.float32, device="cuda:0"), film=torch.zeros(3 * fs.res[0] * fs.res[1], dtype=torch.float32, device="cuda:0"))

    def _render(self, f):
        with torch.cuda.stream(self.stream):
            f["film"].zero_()
        for tl in f["lists"]:
            self.it.render_tile_list_device(self.sc, f["cam"], self.smp, tl, f["slab"].data_ptr(), stream=self.cs)
            tl.update_film_device(f["slab"].data_ptr(), f["fs"].res, f["film"].data_ptr(), stream=self.cs, accumulate=True)

    def full_route(self):
        c, f = self.ctx, self.film[1]
        self._render(f)
        c.render_guides_ids_device(self.sc, self.cam, RES, self.guides.data_ptr(), self.ids.data_ptr(), stream=self.cs)
        c.surface_albedo_device(self.sc, self.ids.data_ptr(), RES, self.albedo.data_ptr(), stream=self.cs)
        c.denoise_device(f["film"].data_ptr(), self.guides.data_ptr(), RES, self.dp, f["td"], f["samples"], self.clean.data_ptr(), stream=self.cs, albedo=self.albedo.data_ptr())
        c.tone_map_device(self.clean.data_ptr(), RES, f["td"], yk.ToneMapType.default(), None, self.clean.data_ptr(), stream=self.cs)

    def low_route(self, s):
        c, f = self.ctx, self.low[s]
        lres = f["fs"].res
        self._render(f)
        c.render_guides_device(self.sc, f["cam"], lres, f["guides"].data_ptr(), stream=self.cs)
        c.render_guides_ids_device(self.sc, self.cam, RES, self.guides.data_ptr(), self.ids.data_ptr(), stream=self.cs)
        c.surface_albedo_device(self.sc, self.ids.data_ptr(), RES, self.albedo.data_ptr(), stream=self.cs)
        c.albedo_mean_device(self.sc, self.ids.data_ptr(), lres, s, f["albedo"].data_ptr(), stream=self.cs)
        c.denoise_device(f["film"].data_ptr(), f["guides"].data_ptr(), lres, self.dp, f["td"], f["samples"], f["clean"].data_ptr(), stream=self.cs, albedo=f["albedo"].data_ptr())
        c.upsample_device(f["clean"].data_ptr(), f["guides"].data_ptr(), lres, self.guides.data_ptr(), f["up"], f["td"], None, self.full.data_ptr(), stream=self.cs, low_albedo=f["albedo"].data_ptr(),
                          albedo=self.albedo.data_ptr())
        c.tone_map_device(self.full.data_ptr(), RES, f["td"], yk.ToneMapType.default(), None, self.full.data_ptr(), stream=self.cs)

    def close(self):
        for f in [self.film[1]] + list(self.low.values()):
            for tl in f["lists"]:
                tl.close()

    def frame_ms(self, call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(self.stream)
        call()
        e1.record(self.stream)
        self.stream.synchronize()
        return e0.elapsed_time(e1)

    def save(self, d, sd):
        """The records of the last low routes and of the full route, for the children."""
        host = lambda t, dtype: t.cpu().numpy().view(dtype)  # noqa: E731
        np.save(os.path.join(d, "guides.npy"), host(self.guides, np.float32))
        np.save(os.path.join(d, "albedo.npy"), host(self.albedo, np.float32))
        np.save(os.path.join(d, "full_film.npy"), host(self.film[1]["film"], np.float32))
        for s, f in self.low.items():
            np.save(os.path.join(d, f"low_s{s}.npy"), host(f["clean"], np.float32))
            np.save(os.path.join(d, f"low_guides_s{s}.npy"), host(f["guides"], np.float32))
            np.save(os.path.join(d, f"low_albedo_s{s}.npy"), host(f["albedo"], np.float32))
        up = self.low[FACTORS[0]]["up"]
        cam = {k: ([float(x) for x in v] if isinstance(v, (tuple, list, np.ndarray)) else (int(v) if k == "fov_axis" else float(v))) for k, v in dict(sd.camera).items()}
        json.dump(dict(sigma_normal=up.sigma_normal, sigma_plane=up.sigma_plane, camera=cam), open(os.path.join(d, "meta.json"), "w"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cfg3")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--direct-lib", default=os.path.join(ROOT, "yuki_amd", "libyuki_hip_direct.so"))
    ap.add_argument("--child", default="", help="(internal) upsample the records saved in this directory and exit")
    ap.add_argument("--beside", action="store_true", help="(internal) the child also reprojects and runs one à-trous iteration")
    ap.add_argument("--bench-this", nargs="*", default=[], help="result lines of separate `bench.py` runs on this build (files), recorded beside the measurements")
    ap.add_argument("--bench-parent", nargs="*", default=[], help="the same of the parent commit's tree, run alternating with them")
    ap.add_argument("--bench-cmd", default="python bench.py --gpus 1 --steps 10 --warmup 3")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    result = dict(tool="tools/upsample_bench.py", scene=a.scene, film=list(RES), texture=[256, 256], factors=list(FACTORS), warmup=a.warmup, launches=a.launches, runs=a.runs,
                  timing="end to end and build comparison: device events; kernels: rocprofv3 --kernel-trace --stats of a child run")
    with tempfile.TemporaryDirectory() as tmp:
        ctx = yk.Context(0)
        sd = scenes.by_name(a.scene)
        sd.materials[len(sd.materials) - 2] = dict(kind=abi.MAT_MATTE, a=(0.55, 0.55, 0.55), c=0.0, tex=0)
        sd.textures = [(0.1 + 0.8 * np.random.default_rng(3).random((256, 256, 3))).astype(np.float32)]
        sc = yk.Scene(ctx, sd)
        stream = torch.cuda.Stream()
        r = Routes(ctx, sd, sc, stream)
        routes = [("full", r.full_route)] + [(f"low_s{s}", (lambda s=s: r.low_route(s))) for s in FACTORS]
        for _, call in routes:  # every shape warmed up
            r.frame_ms(call)
        ms = {name: [] for name, _ in routes}
        for _ in range(a.runs):  # alternating
            for name, call in routes:
                ms[name].append(r.frame_ms(call))
        result["end_to_end_ms"] = {name: dict(runs=[round(t, 3) for t in v], fastest=round(min(v), 3), slowest=round(max(v), 3), median=round(statistics.median(v), 3)) for name, v in ms.items()}
        print("end to end (ms):", {k: v["median"] for k, v in result["end_to_end_ms"].items()}, flush=True)
        r.save(tmp, sd)
        r.close()
        sc.close()
        ctx.close()
        del r
        torch.cuda.empty_cache()
        # the two builds alternating, as fresh processes on the same records
        builds = {"lds": None, "direct": a.direct_lib if os.path.exists(a.direct_lib) else ""}
        cmp_runs = {b: {f"s{s}": [] for s in FACTORS} for b in builds}
        sums = {b: {} for b in builds}
        note = None
        if builds["direct"] == "":
            note = f"not measured: {os.path.relpath(a.direct_lib, ROOT)} is not built (tools/build_variant.sh direct -DYK_UPSAMPLE_DIRECT)"
            del builds["direct"]
        for _ in range(a.runs):  # a child that fails or hangs ends the script here (run_child)
            for b, lib in builds.items():
                got = run_child(a, tmp, lib=lib)
                for s in FACTORS:
                    cmp_runs[b][f"s{s}"].append(round(statistics.median(got[f"s{s}"]), 2))
                    sums[b][f"s{s}"] = got[f"s{s}_checksum"]
        result["lds_against_direct"] = dict(what="median call time (us) of each child run, device events; runs alternate lds, direct", note=note or "measured", runs_us=cmp_runs,
                                            range_us={b: {k: [min(v), max(v)] for k, v in d.items() if v} for b, d in cmp_runs.items()},
                                            outputs_identical=(sums["lds"] == sums.get("direct")) if "direct" in builds and sums.get("direct") else None)
        print("lds against direct:", result["lds_against_direct"]["range_us"], result["lds_against_direct"]["outputs_identical"], flush=True)
        try:  # the last device step; only a trace that cannot be read is "not measured", a failed child still ends the script
            kt, trace_note = kernel_times(a, tmp, os.path.join(tmp, "trace")), None
        except (RuntimeError, KeyError, ValueError) as e:
            kt, trace_note = {}, f"not measured: {e}"
    result["kernel_trace"] = trace_note or "measured"
    result["kernels_us"] = {k: summary(v) for k, v in kt.items()}
    result["bound"] = {}
    for s in FACTORS:
        b = bound_bytes(s)
        entry = dict(bytes=b, hbm_peak_bytes_per_s=HBM_PEAK, bound_us=round(b / HBM_PEAK * 1e6, 2))
        if f"k_upsample_s{s}" in kt:
            med = statistics.median(kt[f"k_upsample_s{s}"])
            entry.update(kernel_us=round(med, 2), time_over_bound=round(med / (b / HBM_PEAK * 1e6), 2), gbytes_per_s=round(b / med * 1e-3, 1))
        result["bound"][f"s{s}"] = entry
    if a.bench_this or a.bench_parent:
        value = lambda path: round(json.load(open(path))["value"], 1)  # noqa: E731
        result["bench_py"] = dict(cmd=a.bench_cmd, unit="Mray/s", note="not measured by this tool: the result lines of separate bench.py runs, this build and the parent commit's tree alternating, handed in with --bench-this / --bench-parent",
                                  this_build=[value(f) for f in a.bench_this], parent_build=[value(f) for f in a.bench_parent])
    print("kernels (us):", {k: v["median_us"] for k, v in result["kernels_us"].items()}, result["bound"], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k != "lds_against_direct"}), flush=True)


if __name__ == "__main__":
    main()
