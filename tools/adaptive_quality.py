"""The sweep behind AdaptiveParams' defaults: the HOST instance of the adaptive rule on oracle films (no GPU).

city-small 64 x 36, Path depth 8, Uniform 128: the 128 accumulating passes are rendered once by the oracle and indexed; the
loop is tests/test_adaptive.py's (select -> take the passes the list names -> fold) with the host instance; the error is
the RMSE of x / (1 + x) against a 1024-spp film (tests/test_denoise.py).  Every row is compared with uniform passes at
ceil(total samples / pixels) samples a pixel.  The chosen row minimises e_adaptive / e_uniform among the rows that keep the
3 x 3 dilation and at least 16 first samples: without them a pixel whose first few samples happen to agree is never
revisited, and on one film that shows as noise between rows (the rows without dilation are in the table to be seen, not to
be chosen).  `bound` is the chosen ratio + 0.05, rounded up to 0.01: what tests/test_adaptive.py and
tests/test_gpu_adaptive.py assert at the defaults.

    python tools/adaptive_quality.py [--out profiles/adaptive_quality.json]
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

MIN_SAMPLES = (4, 8, 16, 32)
ROUND_PASSES = (8, 16)
THRESHOLD = (0.05, 0.1, 0.15, 0.2)
EPSILON = (0.01, 0.05)
DILATE = (False, True)
MIN_SAMPLES_FLOOR = 16  # the defaults are chosen among the rows with dilation and at least this many first samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_quality.json"))
    args = ap.parse_args()
    from test_adaptive import QUALITY, oracle_passes, quality_check
    from yuki_amd import core as yk

    passes, conv = oracle_passes()
    table = []
    for mn, rp, thr, eps, dil in itertools.product(MIN_SAMPLES, ROUND_PASSES, THRESHOLD, EPSILON, DILATE):
        p = yk.AdaptiveParams(min_samples=mn, max_samples=QUALITY["spp"], round_passes=rp, dilate=dil, threshold=thr, epsilon=eps)
        e_ad, e_un, mean_spp, rounds, capped = quality_check(yk, passes, conv, p)
        table.append(dict(min_samples=mn, round_passes=rp, threshold=thr, epsilon=eps, dilate=int(dil), rounds=rounds, mean_spp=round(mean_spp, 2), at_the_cap=round(capped, 3),
                          e_adaptive=round(e_ad, 5), e_uniform=round(e_un, 5), ratio=round(e_ad / e_un, 4)))  # fmt: skip
        print(table[-1], flush=True)
    table.sort(key=lambda r: r["ratio"])
    best = next(r for r in table if r["dilate"] == 1 and r["min_samples"] >= MIN_SAMPLES_FLOOR)
    result = dict(
        what="host instance of the adaptive rule on oracle films; city-small 64 x 36, Path 8, Uniform 128; error = RMSE of x/(1+x) against 1024 spp; uniform at ceil(mean spp)",
        chosen={k: best[k] for k in ("min_samples", "round_passes", "threshold", "epsilon", "dilate")},
        measured_ratio=best["ratio"],
        bound=float(np.ceil((best["ratio"] + 0.05) * 100 - 1e-9) / 100),
        table=table,
    )
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("chosen", result["chosen"], "ratio", best["ratio"], "bound", result["bound"])


if __name__ == "__main__":
    main()
