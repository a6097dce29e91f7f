"""What the guided upsample buys, on oracle films (no GPU): the HOST instance of yk_upsample on textured-city, whose ground
texels are smaller than a pixel at these sizes, and on textured-cornell at 96 x 96, whose texels are far larger than one.

Per (full resolution, s) and per albedo route of tests/test_upsample.py ("centre": the centre ray's record and its s x s
mean; "mean": pixel means over the ids of the 4-times larger film at both resolutions — the 2-times larger one at s = 4, whose
low factor is then the largest the library takes, 8):
  - the ratios tests/test_upsample.py asserts at 96 x 54, s = 2: e_guided / e_bilinear on the whole film and on the mask,
    e_guided / e_geom, the mask's and the fallback's share — the 4-spp low film, denoised, upsampled;
  - the two comparisons a user needs, each raw and after yk_denoise_albedo, against the 1024-spp full film:
      same spp    the upsampled low film (4 spp) against a full-resolution film of 4 spp, which costs s*s times the rays;
      same rays   the upsampled low film of s*s spp against a full-resolution film of 1 spp.
The error is the RMSE of x / (1 + x) (tests/test_denoise.py).  54 is no multiple of 4, so s = 4 runs on the 192 x 108 film of
the same view, and s = 2 there beside it.  Nothing here has a bound.

    python tools/upsample_quality.py [--out profiles/upsample_quality.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = (("textured-city", (96, 54), 2), ("textured-city", (192, 108), 2), ("textured-city", (192, 108), 4), ("textured-cornell", (96, 96), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upsample_quality.json"))
    args = ap.parse_args()
    import albedo_ref as aref
    from oracle import binding as oracle
    from test_denoise import SEED
    from test_upsample import MEAN_S, quality_inputs, quality_ratios
    from yuki_amd import abi
    from yuki_amd import core as yk

    q = aref.QUALITY
    integ = abi.IntegratorDesc(abi.INTEGRATOR_PATH, q["depth"], 0, 0.0)
    err = lambda x, conv: round(aref.quality_error(x, conv), 5)  # noqa: E731

    def render(osc, sd, fs, spp):
        cam, tiles = yk.Camera(sd.camera, fs), yk.film_tiles(fs)
        return yk.update_tiles(tiles, osc.render_tiles(cam.matrices, abi.SamplerDesc(abi.SAMPLER_UNIFORM, spp, 1, 1, SEED), integ, tiles, n_threads=0)[0], fs.res)

    rows = []
    for scene_name, res, s in CASES:
        sd = aref.textured_city() if scene_name == "textured-city" else aref.textured_cornell()
        scene = yk.Scene(None, sd)
        i = scene.info()
        diag = float(np.linalg.norm(np.array(i.bounds_max[:], np.float64) - np.array(i.bounds_min[:], np.float64)))
        dp = yk.DenoiseParams(q["iterations"], q["sigma_color"], q["sigma_normal"], q["plane_fraction"] * diag)
        fs = yk.FilmSettings(res=res, tile_dim=16)
        lfs = yk.subsampled(fs, s)
        mean_s = MEAN_S if s * MEAN_S <= abi.UPSAMPLE_MAX_S else abi.UPSAMPLE_MAX_S // s  # the low factor s * mean_s is at most 8
        low4, conv, low_guides, guides, ids, ids_big = quality_inputs(yk, oracle, sd, res, s, q, mean_s=mean_s)
        osc = oracle.OracleScene(sd)
        full = {spp: render(osc, sd, fs, spp) for spp in (q["noisy_spp"], 1)}
        low = {q["noisy_spp"]: low4, s * s: low4 if s * s == q["noisy_spp"] else render(osc, sd, lfs, s * s)}
        osc.close()
        for route in ("centre", "mean"):
            whole, masked, share, fallback = quality_ratios(yk, oracle, scene, low4, conv, low_guides, guides, ids, ids_big, s, q, route, mean_s=mean_s)
            if route == "centre":
                albedo, low_albedo = yk.surface_albedo(scene, ids), yk.albedo_mean(scene, ids, s)
            else:
                albedo, low_albedo = yk.albedo_mean(scene, ids_big, mean_s), yk.albedo_mean(scene, ids_big, s * mean_s)
            up = yk.UpsampleParams(s, q["sigma_normal"], q["plane_fraction"] * diag)
            kw = dict(low_albedo=low_albedo, albedo=albedo)
            row = dict(scene=scene_name, res=list(res), s=s, low_res=list(lfs.res), albedo=route, mean_s=mean_s if route == "mean" else None, e_guided=round(whole[0], 5), e_geom=round(whole[1], 5), e_bilinear=round(whole[2], 5),
                       guided_over_bilinear=round(whole[0] / whole[2], 4), guided_over_bilinear_masked=round(masked[0] / masked[2], 4), guided_over_geom=round(whole[0] / whole[1], 4),
                       mask_share=round(share, 4), fallback_share=round(fallback, 4))
            for name, low_spp, full_spp in (("same_spp", q["noisy_spp"], q["noisy_spp"]), ("same_rays", s * s, 1)):
                lo, fu = low[low_spp], full[full_spp]
                row[name] = dict(
                    low_spp=low_spp, full_spp=full_spp,
                    raw=dict(upsampled=err(yk.upsample(lo, low_guides, guides, up, **kw), conv), full=err(fu, conv)),
                    denoised=dict(upsampled=err(yk.upsample(yk.denoise(lo, low_guides, dp, albedo=low_albedo), low_guides, guides, up, **kw), conv), full=err(yk.denoise(fu, guides, dp, albedo=albedo), conv)),
                )
                for k in ("raw", "denoised"):
                    row[name][k]["upsampled_over_full"] = round(row[name][k]["upsampled"] / row[name][k]["full"], 4)
            rows.append(row)
            print(row, flush=True)
        scene.close()
    result = dict(tool="tools/upsample_quality.py", depth=q["depth"], converged_spp=q["converged_spp"], denoise=dict(iterations=q["iterations"], sigma_color=q["sigma_color"],
                  sigma_normal=q["sigma_normal"], plane_fraction=q["plane_fraction"]), error="RMSE of x / (1 + x) against the converged full film", instance="host", rows=rows)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
