#!/usr/bin/env python3
"""Meshes moved by matrix: Scene.transform with the records resident (yk_scene_transform_device) against Scene.update with
the pre-transformed tensors resident (yk_scene_update_device) — the path before, MINUS the caller's own transform, so a
lower bound the new call cannot beat: what it adds is the check pass and the write pass over the rest copy.

For each scene (default cfg3 and cfg5, SAH, one shape per leaf): every mesh that carries no area light gets a small rotation
about the vertical axis through the scene's centre and a shift of 1 % of the diagonal, two phases of it taken in turn so that
every call really moves the scene.  After one warm-up of each (the transform's first call keeps the rest copy and builds the
plan: reported on its own), the two alternate on two scenes created alike, `--runs` whole calls each, host clock around
the call (both end synchronised).  Reported: every run with its phase seconds, rest_bytes, the slowest transform against the
fastest update.  Then, on cfg3:

  motion   k_motion_xf (yk_surface_motion_transforms_device, 128 bytes a mesh kept) against k_motion
           (yk_surface_motion_device, the previous vertex tensor kept) on a 1080p film, device events around each call
  cost     one building moved by 0, 0.1 and 1 scene diagonals: tree_cost / tree_cost_rest, the same times the root's area
           (tree_cost is relative to the root, which grows with the move), and one 1920x1080 x 64 spp Path-8 frame, ms

`--kernels-only` runs a few transforms and motion launches and nothing else: the run to put under a kernel trace for the
kernels' own times (the tree-cost pass among them).

    python tools/scene_transform_bench.py --out profiles/scene_transform_device.json
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch  # before the library: one process holds one HIP runtime (tests/conftest.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yuki_amd import abi, scenes  # noqa: E402
from yuki_amd import core as yk  # noqa: E402

from scene_input_bench import tensors  # noqa: E402
from scene_update_bench import frame_ms, timed  # noqa: E402
from temporal_bench import RES, summary  # noqa: E402
from temporal_bench import timed as timed_events  # noqa: E402


def lit_meshes(sd):
    al = np.asarray(sd.tri_area_light) if sd.tri_area_light is not None else np.full(sd.n_triangles, -1)
    tm = np.asarray(sd.tri_mesh) if sd.tri_mesh is not None else np.zeros(sd.n_triangles, np.uint32)
    return set(int(m) for m in np.unique(tm[al >= 0]))


def phase_matrices(sd, phase):
    p = np.asarray(sd.points, np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    centre, diag = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    lit = lit_meshes(sd)
    out = []
    for m in range(len(sd.meshes)):
        if m in lit:
            out.append(None)
            continue
        a = 0.02 * math.sin(0.37 * m + phase)
        r = np.array([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
        mat = np.eye(4)
        mat[:3, :3] = r
        mat[:3, 3] = centre - r @ centre + 0.01 * diag * np.array([math.cos(m + phase), 0.0, math.sin(m + phase)])
        out.append(mat)
    return out


def vertex_meshes(resident, n_vertices, n_meshes):
    """The mesh of every vertex on the device (the smallest mesh of the triangles that index it; n_meshes: none)."""
    idx = resident["indices"].view(-1).long()
    tm = resident["tri_mesh"].view(-1).long().repeat_interleave(3)
    return torch.full((n_vertices,), n_meshes, dtype=torch.long, device="cuda:0").scatter_reduce(0, idx, tm, "amin")


def pre_transformed(rec, vmesh, points, normals):
    """What the caller of Scene.update computes itself (affine records; float32 on the device, not bit-exact: for timing)."""
    m = torch.from_numpy(np.concatenate([rec["rest_to_world"], np.eye(4, dtype=np.float32).reshape(1, 16)]).reshape(-1, 4, 4)).to("cuda:0")[vmesh]
    mi = torch.from_numpy(np.concatenate([rec["world_to_rest"], np.eye(4, dtype=np.float32).reshape(1, 16)]).reshape(-1, 4, 4)).to("cuda:0")[vmesh]
    p = (torch.einsum("vij,vj->vi", m[:, :3, :3], points) + m[:, :3, 3]).contiguous()
    n = None if normals is None else torch.einsum("vji,vj->vi", mi[:, :3, :3], normals).contiguous()
    return p, n


def dev_records(rec):
    return torch.from_numpy(np.ascontiguousarray(rec).view(np.float32).reshape(-1).copy()).to("cuda:0")


def transform_record(s, wall):
    i = s.transform_info()
    assert (i.route, i.reason) == (abi.UPDATE_ROUTE_DEVICE, 0), (i.route, i.reason)
    return dict(transform_seconds=wall, seconds_check=i.seconds_check, seconds_points=i.seconds_points, seconds_boxes=i.seconds_boxes, seconds_records=i.seconds_records, seconds_total=i.seconds_total)


def motion_times(ctx, s, sd, d_prev_records, d_prev_points, launches, warmup):
    fs = yk.FilmSettings(res=RES, tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    n_px = RES[0] * RES[1]
    stream = torch.cuda.Stream()
    cs = stream.cuda_stream
    d_g, d_ids, d_a, d_b = (torch.zeros(k * n_px, dtype=torch.float32, device="cuda:0") for k in (8, 4, 4, 4))
    torch.cuda.synchronize()
    ctx.render_guides_ids_device(s, cam, RES, d_g.data_ptr(), d_ids.data_ptr(), stream=cs)
    stream.synchronize()
    G, I = d_g.data_ptr(), d_ids.data_ptr()
    from_points = timed_events(stream, launches, warmup, lambda: ctx.surface_motion_device(s, I, G, d_prev_points.data_ptr(), RES, d_a.data_ptr(), stream=cs))
    from_records = timed_events(stream, launches, warmup, lambda: ctx.surface_motion_device(s, I, G, None, RES, d_b.data_ptr(), stream=cs, d_prev_transforms_ptr=d_prev_records.data_ptr()))
    same = float((d_a.view(torch.int32) == d_b.view(torch.int32)).float().mean().item())
    return dict(film=list(RES), k_motion=summary(from_points, n_px * 64), k_motion_xf=summary(from_records, n_px * 64), records_equal_fraction=same,
                note="records_equal_fraction compares with the bench's own float32 pre-transform, which is not the rule's arithmetic")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cfg3,cfg5")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = yk.Context(0)
    result = dict(tool="tools/scene_transform_bench.py", split_method="SAH", max_shapes_in_node=1, scenes={})
    for name in a.scenes.split(","):
        sd = scenes.by_name(name)
        sd.split_method, sd.max_shapes_in_node = abi.SPLIT_SAH, 1
        resident = tensors(sd)
        n_v, n_m = int(resident["points"].shape[0]), len(sd.meshes)
        vmesh = vertex_meshes(resident, n_v, n_m)
        recs = [abi.pack_mesh_transforms(phase_matrices(sd, phase)) for phase in (0.0, 1.0)]
        d_recs = [dev_records(r) for r in recs]
        moved = [pre_transformed(r, vmesh, resident["points"], resident.get("normals")) for r in recs]
        out = dict(n_shapes=int(sd.n_triangles), n_vertices=n_v, n_meshes=n_m, records_bytes=int(d_recs[0].numel() * 4), points_bytes=int(n_v * 12), normals=resident.get("normals") is not None)
        s = yk.Scene.from_device(ctx, sd, resident)
        if a.kernels_only:
            for k in range(4):
                s.transform(d_recs[k % 2])
            if name == "cfg3":
                motion_times(ctx, s, sd, d_recs[0], moved[0][0], 5, 1)
            s.close()
            continue
        u = yk.Scene.from_device(ctx, sd, resident)
        _, wall = timed(lambda: s.transform(d_recs[1]))  # the first one keeps the rest copy and builds the plan
        i = s.transform_info()
        out.update(first_transform_seconds=wall, rest_bytes=int(i.rest_bytes), plan_bytes=int(s.update_info().plan_bytes), device_bytes=int(s.info().device_bytes), n_moved_meshes=int(i.n_moved_meshes),
                   tree_cost=i.tree_cost, tree_cost_rest=i.tree_cost_rest)
        u.update(*moved[1])
        rec = dict(transform=[], update=[])
        for k in range(a.runs):
            _, wall = timed(lambda: u.update(*moved[k % 2]))
            iu = u.update_info()
            rec["update"].append(dict(update_seconds=wall, seconds_check=iu.seconds_check, seconds_boxes=iu.seconds_boxes, seconds_records=iu.seconds_records, seconds_total=iu.seconds_total))
            _, wall = timed(lambda: s.transform(d_recs[k % 2]))
            rec["transform"].append(transform_record(s, wall))
            print(f"{name}: #{k} update {rec['update'][-1]['update_seconds'] * 1e3:.3f} ms, transform {wall * 1e3:.3f} ms", flush=True)
        rec["transform_slowest_seconds"] = max(r["transform_seconds"] for r in rec["transform"])
        rec["transform_fastest_seconds"] = min(r["transform_seconds"] for r in rec["transform"])
        rec["update_fastest_seconds"] = min(r["update_seconds"] for r in rec["update"])
        rec["update_slowest_seconds"] = max(r["update_seconds"] for r in rec["update"])
        rec["transform_slowest_over_update_fastest"] = rec["transform_slowest_seconds"] / rec["update_fastest_seconds"]
        out["calls"] = rec
        u.close()
        if name == "cfg3":
            out["motion_1080p"] = motion_times(ctx, s, sd, d_recs[0], moved[0][0], a.launches, 3)
            p = np.asarray(sd.points, np.float64)
            diag = float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))
            free = [m for m in range(n_m) if m not in lit_meshes(sd)][0]
            out["cost_against_frame_time"] = []
            for distance in (0.0, 0.1, 1.0):
                shift = np.eye(4)
                shift[0, 3] = distance * diag
                s.transform(dev_records(abi.pack_mesh_transforms([shift if m == free else None for m in range(n_m)])))
                i, b = s.transform_info(), s.info()
                d = np.array(b.bounds_max[:], np.float64) - np.array(b.bounds_min[:], np.float64)
                area = 2.0 * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0])
                out["cost_against_frame_time"].append(dict(moved_mesh=free, diagonals=distance, tree_cost=i.tree_cost, tree_cost_rest=i.tree_cost_rest, ratio=i.tree_cost / i.tree_cost_rest,
                                                           root_area=area, tree_cost_times_root_area=i.tree_cost * area, frame_1080p_64spp_ms=frame_ms(ctx, s, sd)))
                print(f"{name}: {out['cost_against_frame_time'][-1]}", flush=True)
        s.close()
        result["scenes"][name] = out
        del resident, moved, vmesh
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
