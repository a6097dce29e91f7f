#!/usr/bin/env python3
"""Device time of the motion passes (yk_render_guides_ids_device: k_guides_ids behind the trace, yk_surface_motion_device:
k_motion, yk_history_reproject_moved_device: k_reproject<true>) on a 1080p film, from device events — and, in the same
run, of the two existing entries they stand beside (yk_render_guides_device, yk_history_reproject_device), so that a
change in those shows.

The scene is cfg3 at 1080p under its own camera, which stands.  The history is the blend of a one-sample film the device
rendered of the OLD geometry, with that geometry's guides; then the scene is updated with its points moved by a smooth wave
of `--wobble` x the scene diagonal (area-light vertices stay), and the passes are timed on the new geometry with the old
vertex array as `prev_points`.  After `--warmup` calls, `--launches` calls of each pass, each between its own pair of
events on the caller's stream; reported are the median and the range.
The calls repeat on the same buffers: the times are cache-warm (the largest working set, reproject's 199 MB, fits in the
256 MB last-level cache), as they largely are in use, where the guides, ids and motion records were written just before.
Recorded beside each time: the bytes the pass must at least move and what they take at the 6.29 TB/s copy ceiling.
  guides + ids:     32 + 16 bytes written per pixel (the trace in front of it reads the tree: not counted);
  motion:           16 bytes of id and 32 of guide read, 16 written per pixel (the gather — 12 bytes of indices and 36 of
                    vertices per triangle hit, shared between neighbouring pixels — is reported apart, as requested bytes);
  reproject-moved:  16 bytes of guide and 16 of motion read, 48 bytes of previous record read, 16 written per pixel.

    python tools/motion_bench.py --out profiles/motion_device.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from temporal_bench import COPY_CEILING_GBPS, RES, SEED, summary, timed  # noqa: E402
from yuki_amd import core as yk  # noqa: E402
from yuki_amd import scenes  # noqa: E402

RECORDED_US = dict(render_guides=833.0, reproject=30.5)  # profiles/denoise_device.json, profiles/temporal_device.json


def wobbled(sd, fraction):
    """The points of `sd` moved by a smooth wave of `fraction` of the scene's diagonal; vertices of area-light triangles stay."""
    p = np.ascontiguousarray(sd.points, dtype=np.float32)
    lo, hi = p.min(axis=0), p.max(axis=0)
    ext = np.maximum(hi - lo, np.float32(1e-3))
    amp = np.float32(fraction) * np.float32(np.linalg.norm(hi - lo))
    moved = (p + amp * np.sin(np.float32(3.0 * np.pi) * ((p - lo) / ext)[:, [1, 2, 0]] + np.arange(3, dtype=np.float32))).astype(np.float32)
    al = np.asarray(sd.tri_area_light) if sd.tri_area_light is not None else np.zeros(0, np.int32)
    lit = np.unique(np.asarray(sd.indices)[np.nonzero(al >= 0)[0]].reshape(-1)).astype(np.int64)
    moved[lit] = p[lit]
    return np.ascontiguousarray(moved)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cfg3")
    ap.add_argument("--wobble", type=float, default=0.01)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = yk.Context(0)
    sd = scenes.by_name(a.scene)
    fs = yk.FilmSettings(res=RES, tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    sc = yk.Scene(ctx, sd)
    tiles = yk.film_tiles(fs)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=5)))
    film = yk.update_tiles(tiles, it.render_tiles(sc, cam, yk.SamplerType.Uniform(1, SEED), tiles)[0], fs.res)
    params = yk.TemporalParams.for_scene(sc)
    n_px = RES[0] * RES[1]
    samples = np.ones((-(-RES[0] // 16)) * (-(-RES[1] // 16)), np.uint32)
    stream = torch.cuda.Stream()
    cs = stream.cuda_stream
    z = lambda k: torch.zeros(k, dtype=torch.float32, device="cuda:0")  # noqa: E731
    d_film = torch.from_numpy(film.reshape(-1)).to("cuda:0")
    d_old = torch.from_numpy(np.ascontiguousarray(sd.points, dtype=np.float32)).to("cuda:0")
    d_new = torch.from_numpy(wobbled(sd, a.wobble)).to("cuda:0")
    d_ga, d_gb, d_ids, d_motion, d_hist_a, d_carried, d_plain = z(8 * n_px), z(8 * n_px), z(4 * n_px), z(4 * n_px), z(4 * n_px), z(4 * n_px), z(4 * n_px)
    torch.cuda.synchronize()
    ctx.render_guides_device(sc, cam, RES, d_ga.data_ptr(), stream=cs)
    ctx.blend_history_device(d_film.data_ptr(), RES, params, 16, samples, None, d_hist_a.data_ptr(), None, stream=cs)
    stream.synchronize()

    def report(name, us, moved, **more):
        r = summary(us, moved)
        r.update(more)
        print(name, json.dumps({k: v for k, v in r.items() if k != "launch_us"}), flush=True)
        return r

    G, I, M = d_gb.data_ptr(), d_ids.data_ptr(), d_motion.data_ptr()
    # the geometry as created: what profiles/denoise_device.json timed
    guides_created = report("render_guides, scene as created", timed(stream, a.launches, a.warmup, lambda: ctx.render_guides_device(sc, cam, RES, G, stream=cs)), n_px * 32,
                            recorded_us=RECORDED_US["render_guides"])
    guides_ids_created = report("render_guides_ids, scene as created", timed(stream, a.launches, a.warmup, lambda: ctx.render_guides_ids_device(sc, cam, RES, G, I, stream=cs)), n_px * 48)
    sc.update(d_new)
    route = int(sc.update_info().route)
    # the same two through the refitted tree of the moved geometry
    guides = report("render_guides", timed(stream, a.launches, a.warmup, lambda: ctx.render_guides_device(sc, cam, RES, G, stream=cs)), n_px * 32)
    plain_guides = d_gb.clone()
    guides_ids = report("render_guides_ids", timed(stream, a.launches, a.warmup, lambda: ctx.render_guides_ids_device(sc, cam, RES, G, I, stream=cs)), n_px * 48)
    assert torch.equal(plain_guides.view(torch.int32), d_gb.view(torch.int32))
    hit = d_gb.view(-1, 8)[:, 3] != 0
    tri = hit & (d_ids.view(torch.int32).view(-1, 4)[:, 0] < sd.n_triangles) & (d_ids.view(torch.int32).view(-1, 4)[:, 0] >= 0)
    n_tri = int(tri.sum().item())
    motion = report("surface_motion", timed(stream, a.launches, a.warmup, lambda: ctx.surface_motion_device(sc, I, G, d_old.data_ptr(), RES, M, stream=cs)), n_px * (16 + 32 + 16),
                    gather_bytes_requested=n_tri * 48, hit_fraction=round(float(hit.float().mean().item()), 4), triangle_fraction=round(n_tri / n_px, 4))
    moved_px = (d_motion.view(-1, 4)[:, :3] != d_gb.view(-1, 8)[:, 4:7]).any(1) & hit
    motion.update(pixels_that_moved=round(float(moved_px.float().mean().item()), 4))
    H, GA = d_hist_a.data_ptr(), d_ga.data_ptr()
    plain = report("reproject", timed(stream, a.launches, a.warmup, lambda: ctx.reproject_history_device(H, GA, cam, G, RES, params, d_plain.data_ptr(), stream=cs)), n_px * (32 + 48 + 16),
                   recorded_us=RECORDED_US["reproject"])
    plain.update(pixels_with_history=round(float((d_plain.view(-1, 4)[:, 3] > 0).float().mean().item()), 4))
    moved = report("reproject_moved", timed(stream, a.launches, a.warmup, lambda: ctx.reproject_history_moved_device(H, GA, cam, G, M, RES, params, d_carried.data_ptr(), stream=cs)),
                   n_px * (16 + 16 + 48 + 16))
    moved.update(pixels_with_history=round(float((d_carried.view(-1, 4)[:, 3] > 0).float().mean().item()), 4))
    print("history kept: plain", plain["pixels_with_history"], "moved", moved["pixels_with_history"], flush=True)

    result = dict(tool="tools/motion_bench.py", timing="device events around each call, cache-warm (the calls repeat on the same buffers)", film=list(RES), scene=a.scene, wobble=a.wobble,
                  update_route=route, warmup=a.warmup, launches=a.launches, params=dict(plane_tolerance=params.plane_tolerance, normal_cos_min=params.normal_cos_min, max_history=params.max_history),
                  copy_ceiling_gbps=COPY_CEILING_GBPS, render_guides_scene_as_created=guides_created, render_guides_ids_scene_as_created=guides_ids_created, render_guides=guides, render_guides_ids=guides_ids, surface_motion=motion, reproject=plain, reproject_moved=moved)
    sc.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
