"""What the sphere case of the motion pass buys after a sphere moved: the HOST instances of the temporal chain on oracle
films (no GPU).

glass_balls with matte spheres (white, red, green) at 48 x 48; sphere 0 slides by 0.03 x the scene diagonal along the
camera's side vector (Scene.edit would do that in place).  A 64-spp history of the state before, then 4 frames of 4 spp of
the state after, each rectified (yk_history_rectify at the parameters tests/test_rectify.py asserts at) and folded by
blend_history with max_history 64.  The history is carried three ways:

  with      reproject_history_moved through surface_motion(..., prev_spheres=the table before): the sphere's pixels fetch
            the history of the same surface points;
  without   the same with prev_spheres=None — the pass as it was: a sphere's previous position is its current one;
  restart   no history.

The error is the RMSE of x / (1 + x) against 1024 spp (tests/test_denoise.py) over the pixels whose first hit is the moved
sphere, and over the whole film, after 4 blended frames; three seeds, the worst of them reported beside each.

    python tools/scene_edit_quality.py [--out profiles/scene_edit_quality.json]
"""
import argparse
import copy
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RES = (48, 48)
MOVE = 0.03
SEEDS = (1, 2, 3)
F = np.float32


def error(rgb, conv, mask):
    a, b = rgb.astype(np.float64)[mask], conv.astype(np.float64)[mask]
    return float(np.sqrt(np.mean((a / (1 + a) - b / (1 + b)) ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_edit_quality.json"))
    args = ap.parse_args()
    import scene_edit_ref as ref
    import test_rectify as T
    from oracle import binding as oracle
    from test_motion import oracle_view
    from yuki_amd import abi, scenes
    from yuki_amd import core as yk

    q = T.QUALITY
    before = scenes.glass_balls()
    before.spheres = [dict(s, material=m) for s, m in zip(before.spheres, (0, 2, 3))]
    diag = float(np.linalg.norm(np.asarray(before.points).max(axis=0) - np.asarray(before.points).min(axis=0)))
    c = before.camera
    side = np.cross(np.subtract(c["target"], c["position"]).astype(np.float64), np.array(c["up"], np.float64))
    m = np.eye(4)
    m[:3, 3] = MOVE * diag * side / np.linalg.norm(side)
    after = copy.copy(before)
    after.spheres = [ref.transformed(before.spheres[0], m)] + list(before.spheres[1:])

    fs = yk.FilmSettings(res=RES, tile_dim=16)
    cam = yk.Camera(before.camera, fs)
    tiles = yk.film_tiles(fs)
    integ = abi.IntegratorDesc(abi.INTEGRATOR_PATH, q["depth"], 0, 0.0)
    osc_a, osc_b = oracle.OracleScene(before), oracle.OracleScene(after)

    def render(osc, spp, seed):
        return yk.update_tiles(tiles, osc.render_tiles(cam.matrices, abi.SamplerDesc(abi.SAMPLER_UNIFORM, spp, 1, 1, seed), integ, tiles, n_threads=0)[0], fs.res)

    guides_a, _ = oracle_view(oracle, osc_a, before, cam, RES)
    guides_b, ids_b = oracle_view(oracle, osc_b, after, cam, RES)
    scene = yk.Scene(None, after)
    tparams = yk.TemporalParams.for_scene(scene, normal_cos_min=q["normal_cos_min"], max_history=q["max_history"])
    rparams = yk.RectifyParams(radius=T.TABLE["radius"], gamma=T.TABLE["gamma"])
    points = np.ascontiguousarray(before.points, F)
    motion = {"with": yk.surface_motion(scene, ids_b, guides_b, points, prev_spheres=before.spheres), "without": yk.surface_motion(scene, ids_b, guides_b, points)}
    scene.close()
    on_sphere = (ids_b["shape"] == after.n_triangles) & (guides_b["hit"] != 0)
    everywhere = np.ones_like(on_sphere)
    conv = render(osc_b, q["converged_spp"], T.SEED ^ 0x1234567)
    td = 16
    samples = np.full((-(-RES[0] // td)) * (-(-RES[1] // td)), q["noisy_spp"], np.uint32)
    rows = []
    for seed in SEEDS:
        hist = np.zeros((RES[1], RES[0]), abi.HISTORY_DTYPE)
        hist["rgb"] = render(osc_a, q["history_spp"], (T.SEED ^ 0x777) + 7919 * seed)
        hist["n"] = float(q["history_spp"])
        frames = [render(osc_b, q["noisy_spp"], T.SEED + 977 * k + 7919 * seed) for k in range(1, 5)]
        row = dict(seed=seed)
        for chain in ("with", "without", "restart"):
            rec = None if chain == "restart" else yk.reproject_history_moved(hist, guides_a, cam, guides_b, motion[chain], tparams)
            if rec is not None:
                row[f"{chain}_coverage"] = float((rec["n"][on_sphere] > 0).mean())
            for f in frames:
                film = f * F(q["noisy_spp"])
                if rec is not None:
                    rec = yk.rectify_history(rec, film, rparams, tile_dim=td, samples=samples)
                rgb, rec = yk.blend_history(film, tparams, tile_dim=td, samples=samples, history=rec)
            row[f"{chain}_sphere"] = round(error(rgb, conv, on_sphere), 5)
            row[f"{chain}_film"] = round(error(rgb, conv, everywhere), 5)
        rows.append(row)
        print(row, flush=True)
    worst = {k: max(r[k] for r in rows) for k in rows[0] if k.endswith("_sphere") or k.endswith("_film")}
    result = dict(
        what="host instances on oracle films: glass_balls with matte spheres, 48 x 48, sphere 0 moved by 0.03 x the diagonal sideways; a 64-spp history of the state before, 4 frames of 4 spp after, "
        "rectified at the asserted parameters and blended with max_history 64; error = RMSE of x/(1+x) against 1024 spp over the moved sphere's pixels (_sphere) and the whole film (_film)",
        script="tools/scene_edit_quality.py",
        sphere_pixels=int(on_sphere.sum()),
        rectify=dict(T.TABLE),
        seeds=list(SEEDS),
        rows=rows,
        worst=worst,
        with_over_without_on_sphere=round(worst["with_sphere"] / worst["without_sphere"], 4),
        with_over_restart_on_sphere=round(worst["with_sphere"] / worst["restart_sphere"], 4),
    )
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("worst", worst)


if __name__ == "__main__":
    main()
