#!/usr/bin/env python3
"""Host recursion against the device BVH builder ("bvh_builder" = 1), one process.

For each scene (default cfg3 and cfg5, SAH, one shape per leaf): one warm-up of each builder, then the two
alternating, `--builds` builds each.  Recorded per build: yk_scene_info.build_seconds, the build info's phases and
the wall time of the whole yk_scene_create (host clock around the call, which ends synchronised).  The host
recursion runs with the thread count the machine gives it — it is the baseline.  Every device-built tree is
compared with the host-built one (nodes and shape order, bytes).  `--sweep` first builds each scene once per
small-range limit S (and, with --use-sweep-best, runs the alternating builds with the fastest).

    python tools/bvh_build_bench.py --out profiles/bvh_build_device.json
    python tools/bvh_build_bench.py --scenes cfg5 --builds 1 --no-host      # one device build, e.g. under a kernel trace

`--layout` measures the device scene layout ("scene_layout" = 1) instead: after a warm-up of each, (bvh_builder 1,
scene_layout 0) — the yardstick — and (bvh_builder 1, scene_layout 1) alternate, `--builds` yk_scene_create calls each;
recorded per call: its wall time and the phase split (build, builder phases, layout upload / kernels).  The warm-up
compares the seven device record buffers of the two (bytes).

    python tools/bvh_build_bench.py --layout --out profiles/scene_layout_device.json
"""
import argparse
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yuki_amd import abi, scenes  # noqa: E402
from yuki_amd import core as yk  # noqa: E402

PHASES = ("seconds_upload", "seconds_levels", "seconds_small", "seconds_layout", "seconds_copy_back")


def build(ctx, sd):
    t0 = time.perf_counter()
    s = yk.Scene(ctx, sd)
    wall = time.perf_counter() - t0
    i, bi = s.info(), s.build_info()
    rec = dict(build_seconds=i.build_seconds, scene_create_seconds=wall, upload_seconds=i.upload_seconds, builder=int(bi.builder), reason=int(bi.reason), levels=int(bi.levels),
               small_range=int(bi.small_range), small_ranges=int(bi.small_ranges), n_nodes=int(i.n_nodes), tree_depth=int(i.tree_depth))
    rec.update({k: getattr(bi, k) for k in PHASES})
    return s, rec


def records_digest(s):
    return [hashlib.sha256(s.device_records(name).tobytes()).hexdigest() for name in abi.RECORD_NAMES]


def layout_bench(a):
    """(builder 1, layout 0) against (builder 1, layout 1), alternating, one process."""
    ctxs = {0: yk.Context(0, bvh_builder=1), 1: yk.Context(0, bvh_builder=1, scene_layout=1)}
    result = dict(tool="tools/bvh_build_bench.py --layout", split_method="SAH", max_shapes_in_node=1, scenes={})
    for name in a.scenes.split(","):
        sd = scenes.by_name(name)
        sd.split_method, sd.max_shapes_in_node = abi.SPLIT_SAH, 1
        out = dict(n_shapes=int(sd.n_triangles), layout0=[], layout1=[])

        def create(layout):
            s, rec = build(ctxs[layout], sd)
            li = s.layout_info()
            assert rec["builder"] == 1 and rec["reason"] == 0 and (li.layout, li.reason) == (layout, 0), (rec, li.layout, li.reason)
            rec.update(layout=int(li.layout), layout_seconds_upload=li.seconds_upload, layout_seconds_layout=li.seconds_layout, device_bytes=int(s.info().device_bytes))
            return s, rec

        want = None
        for layout in (0, 1):  # warm-up, and the comparison
            s, _ = create(layout)
            got = records_digest(s)
            assert want is None or got == want, "device-laid records differ from the host-laid ones"
            want = got
            s.close()
        for k in range(a.builds):
            for layout in (0, 1):
                s, rec = create(layout)
                s.close()
                out[f"layout{layout}"].append(rec)
                print(f"{name} layout {layout} #{k}: scene_create {rec['scene_create_seconds']:.4f} s, build {rec['build_seconds']:.4f} s (copy_back {rec['seconds_copy_back']:.4f}), upload {rec['upload_seconds']:.4f} s"
                      f" (layout: upload {rec['layout_seconds_upload']:.4f}, kernels {rec['layout_seconds_layout']:.4f})", flush=True)
        out["layout0_fastest_create_seconds"] = min(r["scene_create_seconds"] for r in out["layout0"])
        out["layout1_slowest_create_seconds"] = max(r["scene_create_seconds"] for r in out["layout1"])
        out["layout1_slowest_below_layout0_fastest"] = out["layout1_slowest_create_seconds"] < out["layout0_fastest_create_seconds"]
        result["scenes"][name] = out
    return result


def digest(s):
    n, o = s.export_bvh()
    return hashlib.sha256(n.tobytes()).hexdigest() + hashlib.sha256(o.tobytes()).hexdigest()


def write(result, path):
    print(json.dumps(result))
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cfg3,cfg5")
    ap.add_argument("--builds", type=int, default=5)
    ap.add_argument("--sweep", default="", help="comma-separated small-range limits to try first, e.g. 0,8,16,32,64,128")
    ap.add_argument("--small-range", type=int, default=-1, help="small-range limit of the alternating runs (default: the library's)")
    ap.add_argument("--use-sweep-best", action="store_true", help="run the alternating builds with the sweep's fastest limit instead")
    ap.add_argument("--no-host", action="store_true", help="device builds only (no baseline, no comparison)")
    ap.add_argument("--layout", action="store_true", help='measure "scene_layout" = 1 against 0, both on a device-built tree')
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.layout:
        write(layout_bench(a), a.out)
        return
    host_ctx, dev_ctx = yk.Context(0), yk.Context(0)
    dev_ctx.set_option("bvh_builder", 1)
    result = dict(tool="tools/bvh_build_bench.py", split_method="SAH", max_shapes_in_node=1, scenes={})
    for name in a.scenes.split(","):
        sd = scenes.by_name(name)
        sd.split_method, sd.max_shapes_in_node = abi.SPLIT_SAH, 1
        out = dict(n_shapes=int(sd.n_triangles), sweep=[], host=[], device=[])
        want = None
        if not a.no_host:
            s, _ = build(host_ctx, sd)  # warm-up; its tree is the yardstick
            want = digest(s)
            s.close()
        s, rec = build(dev_ctx, sd)  # warm-up
        assert rec["builder"] == 1 and rec["reason"] == 0, rec
        assert want is None or digest(s) == want, "device-built tree differs from the host-built one"
        s.close()
        for S in [int(x) for x in a.sweep.split(",") if x]:
            dev_ctx.set_option("bvh_small_range", S)
            s, rec = build(dev_ctx, sd)
            assert rec["builder"] == 1 and rec["reason"] == 0, rec
            assert want is None or digest(s) == want, f"S={S}: device-built tree differs from the host-built one"
            s.close()
            out["sweep"].append(rec)
            print(f"{name} sweep S={S}: build {rec['build_seconds']:.4f} s (levels {rec['seconds_levels']:.4f}, small {rec['seconds_small']:.4f}, {rec['levels']} levels)", flush=True)
        if out["sweep"]:
            out["sweep_best_small_range"] = min(out["sweep"], key=lambda r: r["build_seconds"])["small_range"]
            dev_ctx.close()
            dev_ctx = yk.Context(0, bvh_builder=1)  # back to the library's default limit
        chosen = out["sweep_best_small_range"] if a.use_sweep_best and out["sweep"] else a.small_range
        if chosen >= 0:
            dev_ctx.set_option("bvh_small_range", chosen)
        for k in range(a.builds):
            for which, ctx in (("host", host_ctx), ("device", dev_ctx)):
                if which == "host" and a.no_host:
                    continue
                s, rec = build(ctx, sd)
                assert rec["builder"] == (1 if which == "device" else 0) and rec["reason"] == 0, rec
                if which == "device" and want is not None and k == 0:
                    assert digest(s) == want
                s.close()
                out[which].append(rec)
                print(f"{name} {which} #{k}: build {rec['build_seconds']:.4f} s, scene_create {rec['scene_create_seconds']:.4f} s " + " ".join(f"{p[8:]}={rec[p]:.4f}" for p in PHASES if which == "device"), flush=True)
        out["small_range"] = out["device"][0]["small_range"]
        if out["host"]:
            out["host_fastest_build_seconds"] = min(r["build_seconds"] for r in out["host"])
            out["device_slowest_build_seconds"] = max(r["build_seconds"] for r in out["device"])
            out["device_slowest_below_host_fastest"] = out["device_slowest_build_seconds"] < out["host_fastest_build_seconds"]
        result["scenes"][name] = out
    write(result, a.out)


if __name__ == "__main__":
    main()
