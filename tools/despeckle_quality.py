"""The sweep behind DespeckleParams' defaults: the HOST instance of yk_despeckle on oracle films (no GPU).

The three scenes of tests/test_despeckle.py (cornell 48 x 48, city-small 64 x 36, glass-balls 48 x 48; Path depth 8, Uniform
4 spp, frame seeds SEED + 977 k, a 1024-spp film at SEED ^ 0x1234567); the error is the RMSE of x / (1 + x) against the
1024-spp film (tests/test_denoise.py).  For every (radius, rank, gain) of radius 1-2 x rank 1-3 x gain 1, 1.5, 2, 3, 4 the
table holds, per scene:
  - the error of the mean of eight frames, raw and with every frame despeckled, and their ratio;
  - one denoised frame (3 iterations, 4.0 / 0.3 / 0.06) with and without the pass in front, the worst of three seeds;
  - the pixels clamped and the luminance kept per 4-spp frame;
  - the same on the 1024-spp film, and the error of the despeckled 1024-spp film against itself: the BIAS, recorded and
    asserted nowhere;
and, at the chosen row only, for the two cornell chains of tests/test_rectify.py (a lighting change, a camera move), the
rectified and the plain chain with every frame despeckled first beside the chains as they are — recorded, not asserted.
The chosen row has the least mean of e_despeckled / e_raw over the three 8-frame cases.  The bounds of
test_despeckle.test_quality_of_the_despeckled_mean are the midpoints of 1 and the chosen row's ratios.

    python tools/despeckle_quality.py [--out profiles/despeckle_quality.json]
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

RADIUS = (1, 2)
RANK = (1, 2, 3)
GAIN = (1.0, 1.5, 2.0, 3.0, 4.0)
STATED = (1, 1, 2.0)  # the row the pass was proposed with


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "despeckle_quality.json"))
    args = ap.parse_args()
    import test_despeckle as T
    import test_rectify as TR
    from yuki_amd import core as yk

    rows = {}
    for name in T.QUALITY_SCENES:
        frames, conv, guides = T.oracle_films(name)
        for radius, rank, gain in itertools.product(RADIUS, RANK, GAIN):
            p = yk.DespeckleParams(radius=radius, rank=rank, gain=gain)
            e_raw, e_des, n_clamped, kept = T.mean_errors(yk, frames, conv, p)
            e_plain, e_both, ratio = T.denoised_errors(yk, frames, conv, guides, p)
            b_n, b_kept, b_err = T.bias(yk, conv, p)
            rows.setdefault((radius, rank, gain), {})[name] = dict(
                mean8=dict(raw=round(e_raw, 5), despeckled=round(e_des, 5), ratio=round(e_des / e_raw, 5)),
                denoised_frame=dict(denoised=round(e_plain, 5), despeckled_denoised=round(e_both, 5), ratio=round(ratio, 4)),
                frame=dict(clamped_pixels=round(n_clamped, 2), luminance_kept=round(kept, 4)),
                bias_1024spp=dict(clamped_pixels=b_n, luminance_kept=round(b_kept, 4), error_against_itself=round(b_err, 5)),
            )
        print(name, "done", flush=True)
    table = [dict(radius=k[0], rank=k[1], gain=k[2], mean_ratio=round(float(np.mean([c["mean8"]["ratio"] for c in cells.values()])), 5), scenes=cells) for k, cells in rows.items()]
    table.sort(key=lambda r: (r["mean_ratio"], r["radius"], r["rank"], r["gain"]))  # a tie goes to the smaller window, rank and gain
    best = table[0]
    stated = next(r for r in table if (r["radius"], r["rank"], r["gain"]) == STATED)
    chosen = yk.DespeckleParams(radius=best["radius"], rank=best["rank"], gain=best["gain"])

    chains = {}
    for name in ("cornell-lighting", "cornell-camera"):
        tparams, films, moved = TR.oracle_case(name)
        history_film, guides_a, cam_a, guides_b, frames, conv = films
        clean = [yk.despeckle(f, chosen) for f in frames]
        as_is = TR.quality_chains(yk, tparams, films, moved, yk.RectifyParams())
        first = TR.quality_chains(yk, tparams, (history_film, guides_a, cam_a, guides_b, clean, conv), moved, yk.RectifyParams())
        chains[name] = dict(frames=list(TR.QUALITY["frames"]), as_they_are={k: [round(v, 5) for v in e] for k, e in as_is.items()}, despeckled_first={k: [round(v, 5) for v in e] for k, e in first.items()})
        print(name, "done", flush=True)

    result = dict(
        what="host instance of yk_despeckle on oracle films; error = RMSE of x/(1+x) against 1024 spp; frames of 4 spp (seeds SEED + 977 k for frame k = 1 .. 8); min_taps 3, floor 0, no repair",
        scenes={k: list(v) for k, v in T.QUALITY_SCENES.items()},
        chosen=dict(radius=best["radius"], rank=best["rank"], gain=best["gain"], mean_ratio=best["mean_ratio"]),
        chosen_ratio={k: v["mean8"]["ratio"] for k, v in best["scenes"].items()},
        chosen_bound={k: round((1.0 + v["mean8"]["ratio"]) / 2.0, 4) for k, v in best["scenes"].items()},
        chosen_denoised_frame_ratio={k: v["denoised_frame"]["ratio"] for k, v in best["scenes"].items()},
        stated_row=dict(radius=STATED[0], rank=STATED[1], gain=STATED[2], scenes=stated["scenes"]),
        rectify_chains_at_chosen=chains,
        table=table,
    )
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    for r in table:
        print(r["radius"], r["rank"], r["gain"], r["mean_ratio"], {k: v["mean8"]["ratio"] for k, v in r["scenes"].items()})
    print("chosen", result["chosen"], "ratios", result["chosen_ratio"], "bounds", result["chosen_bound"], "denoised frame", result["chosen_denoised_frame_ratio"])
    print("stated row", {k: (v["mean8"], v["frame"]) for k, v in stated["scenes"].items()})


if __name__ == "__main__":
    main()
