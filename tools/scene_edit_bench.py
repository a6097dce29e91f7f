#!/usr/bin/env python3
"""An edited scene: editing it in place (Scene.edit, yk_scene_apply_edit[_device]) against creating it again
(Scene.from_device of the edited description, the only way before), one process, from tensors that are resident before the
clock starts.

  lights    on each scene of --scenes (default cfg3 and cfg5, SAH, one shape per leaf): every light's intensity scaled, two
            values taken in turn so that every edit really changes the table.
  spheres   on a sphere-heavy scene — the Cornell box with a sphere at every vertex of the existing cube-sphere generator
            (scenes._cube_sphere(--cube), 6 n^2 + 2 of them: 101,402 at the default 130) — every sphere translated, two
            offsets taken in turn, the table resident on the device as a tensor of yk_sphere_desc records.

After one warm-up of each (a sphere edit's warm-up builds the update plan; that first call is reported on its own), the two
alternate, `--runs` calls each, and the wall time of the whole call is taken (host clock around it; both end synchronised).
A re-creation packs the description's small tables in Python on every call, an edit only the tables it is given: both are
what a caller of this package pays; the sphere case reports the packing on its own (description_pack_seconds).  Reported per case: every run with the edit's phase seconds and what it rewrote, the
slowest edit against the fastest re-creation (yk_scene_update's verdict rule).

    python tools/scene_edit_bench.py --out profiles/scene_edit_device.json
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch  # before the library: one process holds one HIP runtime (tests/conftest.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yuki_amd import abi, scenes  # noqa: E402
from yuki_amd import core as yk  # noqa: E402

from scene_input_bench import tensors  # noqa: E402


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def edit_record(s, wall):
    i = s.edit_info()
    return dict(edit_seconds=wall, route=int(i.route), reason=int(i.reason), rewrote=int(i.rewrote), seconds_check=i.seconds_check, seconds_tables=i.seconds_tables, seconds_boxes=i.seconds_boxes,
                seconds_records=i.seconds_records, seconds_total=i.seconds_total)


def verdict(rec):
    rec["edit_slowest_seconds"] = max(r["edit_seconds"] for r in rec["edit"])
    rec["edit_fastest_seconds"] = min(r["edit_seconds"] for r in rec["edit"])
    rec["recreate_fastest_seconds"] = min(r["scene_create_seconds"] for r in rec["recreate"])
    rec["edit_slowest_over_recreate_fastest"] = rec["edit_slowest_seconds"] / rec["recreate_fastest_seconds"]
    rec["slowest_edit_below_fastest_recreation"] = rec["edit_slowest_seconds"] < rec["recreate_fastest_seconds"]
    return rec


def scaled_lights(sd, factor):
    if sd.light_structs is not None:
        out = []
        for l in sd.light_structs:
            c = abi.LightDesc.from_buffer_copy(bytes(l))
            c.i = abi.f3([factor * x for x in l.i])
            out.append(c)
        return out
    out = copy.deepcopy(sd.lights)
    for l in out:
        for key in ("L", "I"):
            if key in l:
                l[key] = tuple(factor * float(x) for x in l[key])
    return out


def with_lights(sd, lights):
    out = copy.copy(sd)
    if sd.light_structs is not None:
        out.light_structs = lights
    else:
        out.lights = lights
    return out


def lights_case(ctx, name, runs):
    sd = scenes.by_name(name)
    sd.split_method, sd.max_shapes_in_node = abi.SPLIT_SAH, 1
    resident = tensors(sd)
    tables = [scaled_lights(sd, f) for f in (0.5, 2.0)]
    s, wall = timed(lambda: yk.Scene.from_device(ctx, sd, resident))
    rec = dict(n_shapes=int(sd.n_triangles + len(sd.spheres)), n_lights=len(tables[0]), create_seconds=wall, edit=[], recreate=[])
    s.edit(lights=tables[1])  # warm-up
    yk.Scene.from_device(ctx, with_lights(sd, tables[1]), resident).close()
    for k in range(runs):
        t = tables[k % 2]
        fresh, wall = timed(lambda: yk.Scene.from_device(ctx, with_lights(sd, t), resident))
        fresh.close()
        rec["recreate"].append(dict(scene_create_seconds=wall))
        _, wall = timed(lambda: s.edit(lights=t))
        rec["edit"].append(edit_record(s, wall))
        print(f"{name} lights: #{k} re-create {rec['recreate'][-1]['scene_create_seconds']:.4f} s, edit {wall:.6f} s", flush=True)
    s.close()
    del resident
    torch.cuda.empty_cache()
    return verdict(rec)


def sphere_scene(cube):
    """The Cornell box with a matte sphere at every vertex of the cube-sphere, scaled into the box."""
    sd = scenes.cornell()
    unit, _ = scenes._cube_sphere(cube)
    centre, radius = np.array([0.278, 0.273, -0.28]), 0.22
    at = (centre + radius * np.asarray(unit, np.float64)).astype(np.float32)
    r = float(np.float32(0.6 * radius * np.pi / (2.0 * cube)))  # neighbours do not quite touch
    spheres = []
    for p in at:
        o2w, w2o = scenes._translation(p)
        spheres.append(dict(o2w=o2w, w2o=w2o, radius=r, material=int(len(spheres) % 4)))
    sd.spheres = spheres
    sd.split_method, sd.max_shapes_in_node = abi.SPLIT_SAH, 1
    sd.name = f"cornell-{len(spheres)}-spheres"
    return sd


def moved_records(records, offset):
    out = records.copy()
    out["object_to_world"][:, [3, 7, 11]] += np.asarray(offset, np.float32)
    out["world_to_object"][:, [3, 7, 11]] -= np.asarray(offset, np.float32)
    return out


def spheres_case(ctx, cube, runs):
    sd = sphere_scene(cube)
    resident = tensors(sd)
    records = abi.pack_spheres(sd.spheres)
    host = [moved_records(records, o) for o in ((0.004, 0.002, -0.003), (-0.003, 0.004, 0.002))]
    device = [torch.from_numpy(h.view(np.uint8).copy()).to("cuda:0") for h in host]

    def described(h):  # the description of the moved scene (made outside the clock: a caller has it)
        out = copy.copy(sd)
        out.spheres = [dict(s, o2w=h["object_to_world"][k].reshape(4, 4), w2o=h["world_to_object"][k].reshape(4, 4)) for k, s in enumerate(sd.spheres)]
        return out

    moved_sd = [described(h) for h in host]
    s, wall = timed(lambda: yk.Scene.from_device(ctx, sd, resident))
    rec = dict(scene=sd.name, n_shapes=int(sd.n_triangles + len(sd.spheres)), n_spheres=len(sd.spheres), table_bytes=int(records.nbytes), create_seconds=wall, edit=[], recreate=[])
    _, wall = timed(lambda: s.edit(spheres=device[1]))  # warm-up; the scene's first one builds the plan
    rec.update(first_edit_seconds=wall, plan_bytes=int(s.update_info().plan_bytes), n_levels=int(s.update_info().n_levels))
    yk.Scene.from_device(ctx, moved_sd[1], resident).close()
    _, wall = timed(lambda: moved_sd[0].desc(yk.LightFactory))  # what of a re-creation is the packing of the description in Python
    rec["description_pack_seconds"] = wall
    for k in range(runs):
        fresh, wall = timed(lambda: yk.Scene.from_device(ctx, moved_sd[k % 2], resident))
        fresh.close()
        rec["recreate"].append(dict(scene_create_seconds=wall))
        _, wall = timed(lambda: s.edit(spheres=device[k % 2]))
        rec["edit"].append(edit_record(s, wall))
        assert rec["edit"][-1]["route"] == abi.UPDATE_ROUTE_DEVICE and rec["edit"][-1]["reason"] == 0
        print(f"{sd.name}: #{k} re-create {rec['recreate'][-1]['scene_create_seconds']:.4f} s, edit {wall:.6f} s", flush=True)
    # the motion pass with spheres, once, for the kernel trace: a 256 x 256 view of the edited scene
    fs = yk.FilmSettings(res=(256, 256), tile_dim=16)
    guides, ids = yk.render_guides_ids(ctx, s, yk.Camera(sd.camera, fs), fs)
    _, wall = timed(lambda: yk.surface_motion(s, ids, guides, np.ascontiguousarray(sd.points, np.float32), ctx=ctx, prev_spheres=host[(runs - 1) % 2 ^ 1]))
    rec["surface_motion_spheres_256x256_host_arrays_seconds"] = wall
    s.close()
    return verdict(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cfg3,cfg5")
    ap.add_argument("--cube", type=int, default=130)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = yk.Context(0)
    result = dict(tool="tools/scene_edit_bench.py", split_method="SAH", max_shapes_in_node=1, lights={}, spheres={})
    for name in [n for n in a.scenes.split(",") if n]:
        result["lights"][name] = lights_case(ctx, name, a.runs)
    if a.cube:
        result["spheres"] = spheres_case(ctx, a.cube, a.runs)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
