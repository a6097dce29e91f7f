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


def digest(s):
    n, o = s.export_bvh()
    return hashlib.sha256(n.tobytes()).hexdigest() + hashlib.sha256(o.tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cfg3,cfg5")
    ap.add_argument("--builds", type=int, default=5)
    ap.add_argument("--sweep", default="", help="comma-separated small-range limits to try first, e.g. 0,8,16,32,64,128")
    ap.add_argument("--small-range", type=int, default=-1, help="small-range limit of the alternating runs (default: the library's)")
    ap.add_argument("--use-sweep-best", action="store_true", help="run the alternating builds with the sweep's fastest limit instead")
    ap.add_argument("--no-host", action="store_true", help="device builds only (no baseline, no comparison)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
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
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
