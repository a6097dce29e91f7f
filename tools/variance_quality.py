"""The sweep behind VarianceParams' defaults: the HOST instance of the variance-guided denoise on oracle films (no GPU).

city-small 64 x 36 and cornell 48 x 48; 1, 2, 4 and 8 frames of 4 spp folded by blend_history / blend_moments, against a
1024-spp film; 3 and 5 iterations; the error is the RMSE of x / (1 + x) (tests/test_denoise.py).  For every
(sigma_variance, spatial_scale, epsilon) the table holds the error of the unfiltered blend, of plain yk_denoise at
tests/test_denoise.py's parameters and of the variance-guided filter.  The chosen row minimises the mean over both scenes,
the four frame counts and both iteration counts of e_var / e_blended.

    python tools/variance_quality.py [--out profiles/variance_quality.json]
"""
import argparse
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED = 0x73B9642E74AC471C
SCENES = (("city-small", (64, 36)), ("cornell", (48, 48)))
FRAMES = (1, 2, 4, 8)
ITERATIONS = (3, 5)
SIGMA_VARIANCE = (2.0, 3.0, 4.0, 6.0, 8.0)
SPATIAL_SCALE = (0.25, 1.0, 2.0, 4.0)
EPSILON = (1e-8, 1e-5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variance_quality.json"))
    args = ap.parse_args()
    from oracle import binding as oracle
    from test_denoise import QUALITY as PLAIN
    from test_denoise import oracle_guides, quality_error
    from yuki_amd import abi, scenes
    from yuki_amd import core as yk

    tp = yk.TemporalParams(max_history=64.0)
    rows = {}
    base = {}
    for name, res in SCENES:
        sd = scenes.cornell() if name == "cornell" else scenes.by_name(name)
        fs = yk.FilmSettings(res=res, tile_dim=16)
        cam = yk.Camera(sd.camera, fs)
        tiles = yk.film_tiles(fs)
        osc = oracle.OracleScene(sd)
        integ = abi.IntegratorDesc(abi.INTEGRATOR_PATH, 8, 0, 0.0)
        render = lambda spp, seed: yk.update_tiles(tiles, osc.render_tiles(cam.matrices, abi.SamplerDesc(abi.SAMPLER_UNIFORM, spp, 1, 1, seed), integ, tiles, n_threads=0)[0], fs.res)  # noqa: E731
        frames = [render(4, SEED + 977 * k) for k in range(max(FRAMES))]
        conv = render(1024, SEED ^ 0x1234567)
        guides = oracle_guides(oracle, osc, cam, fs.res)
        host_scene = yk.Scene(None, sd)
        sp = yk.DenoiseParams.for_scene(host_scene).sigma_plane
        host_scene.close()
        hist = mom = None
        for k, f in enumerate(frames, 1):
            rgb, hist = yk.blend_history(f, tp, history=hist)
            mom = yk.blend_moments(f, tp, moments=mom)
            if k not in FRAMES:
                continue
            e_blend = quality_error(rgb, conv)
            e_plain = quality_error(yk.denoise(rgb, guides, yk.DenoiseParams(PLAIN["iterations"], PLAIN["sigma_color"], PLAIN["sigma_normal"], sp)), conv)
            base[f"{name}/{k}"] = dict(blended=round(e_blend, 5), plain=round(e_plain, 5))
            print(name, k, "frames: blended", round(e_blend, 4), "plain", round(e_plain, 4), flush=True)
            for sv, sc, eps, it in itertools.product(SIGMA_VARIANCE, SPATIAL_SCALE, EPSILON, ITERATIONS):
                vp = yk.VarianceParams(iterations=it, sigma_variance=sv, sigma_plane=sp, epsilon=eps, spatial_scale=sc)
                var = yk.variance(mom, rgb, guides, vp)
                e = quality_error(yk.denoise(rgb, guides, vp, variance=var), conv)
                rows.setdefault((sv, sc, eps), {})[f"{name}/{k}/it{it}"] = dict(e=round(e, 5), over_blended=round(e / e_blend, 4), over_plain=round(e / e_plain, 4))
    table = []
    for (sv, sc, eps), cells in rows.items():
        score = float(np.mean([c["over_blended"] for c in cells.values()]))
        table.append(dict(sigma_variance=sv, spatial_scale=sc, epsilon=eps, mean_over_blended=round(score, 4), cells=cells))
    table.sort(key=lambda r: r["mean_over_blended"])
    best = table[0]
    ratio = best["cells"]["city-small/4/it3"]["over_plain"]
    result = dict(
        what="host instance of yk_denoise_variance on oracle films; error = RMSE of x/(1+x) against 1024 spp; frames of 4 spp",
        plain=dict(iterations=PLAIN["iterations"], sigma_color=PLAIN["sigma_color"], sigma_normal=PLAIN["sigma_normal"], sigma_plane="0.01 x scene diagonal"),
        baselines=base,
        chosen=dict(sigma_variance=best["sigma_variance"], spatial_scale=best["spatial_scale"], epsilon=best["epsilon"]),
        measured_ratio=ratio,
        bound=float(np.ceil((ratio + 0.05) * 100 - 1e-9) / 100),
        table=table,
    )
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("chosen", result["chosen"], "ratio", ratio, "bound", result["bound"])


if __name__ == "__main__":
    main()
