#!/usr/bin/env python3
"""A moved mesh: updating the scene in place (Scene.update, yk_scene_update_device) against creating it again
(Scene.from_device, the only way before), one process, from tensors that are resident before the clock starts.

For each scene (default cfg3 and cfg5, SAH, one shape per leaf) and each deformation — a smooth wobble of 1 % and of 10 %
of the scene's diagonal, two phases of it taken in turn so that every update really moves the mesh — after one warm-up
of each (the update's warm-up builds its plan; that first call is reported on its own), the two alternate, `--runs` calls
each, and the wall time of the whole call is taken (host clock around it; both end synchronised).  Reported per scene and
deformation: every run with the update's phase seconds, the plan's bytes and levels, the slowest update against the
fastest re-creation.  Then, on the same scene:

  level pass   seconds_boxes (leaves, the levels, the 32-byte read-back of the root) with "update_top_block" 1 — the top
               levels of at most 256 nodes finished by one block — and 0 — one launch per level throughout
  frame        (cfg3 only) one 1920x1080 x 64 spp Path-8 frame through the refitted tree and through a rebuilt tree of the
               same moved geometry, ms each: what a refit costs in traversal.  For information.

    python tools/scene_update_bench.py --out profiles/scene_update_device.json
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch  # before the library: one process holds one HIP runtime (tests/conftest.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yuki_amd import abi, scenes  # noqa: E402
from yuki_amd import core as yk  # noqa: E402

from scene_input_bench import tensors  # noqa: E402


def wobble(points, fraction, phase):
    """tests/test_scene_update.py's wave, on the device (the bench scenes have no area-light triangles to hold still)."""
    lo, hi = points.min(dim=0).values, points.max(dim=0).values
    ext = torch.clamp(hi - lo, min=1e-3)
    amp = fraction * float(torch.linalg.norm(hi - lo))
    u = (points - lo) / ext
    shift = torch.arange(3, dtype=torch.float32, device=points.device) + phase
    return (points + amp * torch.sin(3.0 * math.pi * u[:, [1, 2, 0]] + shift)).contiguous()


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    return r, time.perf_counter() - t0


def update_record(s, wall):
    i = s.update_info()
    assert (i.route, i.reason) == (abi.UPDATE_ROUTE_DEVICE, 0), (i.route, i.reason)
    return dict(update_seconds=wall, seconds_check=i.seconds_check, seconds_boxes=i.seconds_boxes, seconds_records=i.seconds_records, seconds_total=i.seconds_total)


def frame_ms(ctx, scene, sd, runs=3):
    fs = yk.FilmSettings(res=(1920, 1080), tile_dim=16)
    integ = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=8)))
    cam, sampler, tiles = yk.Camera(sd.camera, fs), yk.SamplerType.Stratified((8, 8), True), yk.film_tiles(fs)
    out = torch.zeros((1920 * 1080, 3), dtype=torch.float32, device="cuda:0")
    best = None
    for _ in range(runs + 1):  # the first one warms up
        _, wall = timed(lambda: integ.render_tiles_device(scene, cam, sampler, tiles, out.data_ptr()))
        best = wall if best is None else min(best, wall)
    return 1e3 * best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cfg3,cfg5")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = yk.Context(0)
    result = dict(tool="tools/scene_update_bench.py", split_method="SAH", max_shapes_in_node=1, scenes={})
    for name in a.scenes.split(","):
        sd = scenes.by_name(name)
        sd.split_method, sd.max_shapes_in_node = abi.SPLIT_SAH, 1
        resident = tensors(sd)
        out = dict(n_shapes=int(sd.n_triangles), points_bytes=int(resident["points"].numel() * 4), deformations={})
        s, wall = timed(lambda: yk.Scene.from_device(ctx, sd, resident))
        out["create_seconds"] = wall
        for fraction in (0.01, 0.1):
            moved = [wobble(resident["points"], fraction, phase) for phase in (0.0, 1.0)]
            rec = dict(update=[], recreate=[])
            _, wall = timed(lambda: s.update(moved[1]))  # warm-up; the scene's first one builds the plan
            i = s.update_info()
            if "first_update_seconds" not in out:
                out.update(first_update_seconds=wall, plan_bytes=int(i.plan_bytes), n_levels=int(i.n_levels), device_bytes=int(s.info().device_bytes))
            yk.Scene.from_device(ctx, sd, dict(resident, points=moved[1])).close()
            for k in range(a.runs):
                m = moved[k % 2]
                fresh, wall = timed(lambda: yk.Scene.from_device(ctx, sd, dict(resident, points=m)))
                fresh.close()
                rec["recreate"].append(dict(scene_create_seconds=wall))
                _, wall = timed(lambda: s.update(m))
                rec["update"].append(update_record(s, wall))
                print(f"{name} {fraction}: #{k} re-create {rec['recreate'][-1]['scene_create_seconds']:.4f} s, update {wall:.4f} s", flush=True)
            rec["update_slowest_seconds"] = max(r["update_seconds"] for r in rec["update"])
            rec["update_fastest_seconds"] = min(r["update_seconds"] for r in rec["update"])
            rec["recreate_fastest_seconds"] = min(r["scene_create_seconds"] for r in rec["recreate"])
            rec["update_slowest_over_recreate_fastest"] = rec["update_slowest_seconds"] / rec["recreate_fastest_seconds"]
            out["deformations"][str(fraction)] = rec
        # the level pass with and without the one-block top, on the 10 % wobble
        out["level_pass"] = {}
        for top_block in (1, 0, 1, 0):
            ctx.set_option("update_top_block", top_block)
            runs = []
            for k in range(a.runs):
                _, wall = timed(lambda: s.update(moved[k % 2]))
                runs.append(s.update_info().seconds_boxes)
            out["level_pass"].setdefault(f"top_block_{top_block}_seconds_boxes", []).extend(runs)
        for key in list(out["level_pass"]):
            out["level_pass"][key.replace("seconds_boxes", "median")] = float(np.median(out["level_pass"][key]))
        ctx.set_option("update_top_block", 1)
        if name == "cfg3":  # one frame through the refitted tree (s holds moved[1 - runs % 2] ...) and through a rebuilt one
            s.update(moved[1])
            rebuilt = yk.Scene.from_device(ctx, sd, dict(resident, points=moved[1]))
            out["frame_1080p_64spp_ms"] = dict(deformation=0.1, refitted_tree=frame_ms(ctx, s, sd), rebuilt_tree=frame_ms(ctx, rebuilt, sd))
            rebuilt.close()
            print(f"{name}: frame {out['frame_1080p_64spp_ms']}", flush=True)
        s.close()
        result["scenes"][name] = out
        del resident, moved
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
