"""The sweep behind RectifyParams' defaults: the HOST instance of yk_history_rectify on oracle films (no GPU).

The three cases of tests/test_rectify.py (cornell 48 x 48 after a lighting change under a still camera, cornell after a
camera move of 0.03 x the scene diagonal, city-small 64 x 36 after a move of 0.01 x the diagonal): a 64-spp history of the
state before the change, then 1, 2, 4 and 8 frames of 4 spp of the state after it, folded by blend_history with
max_history 64; the error is the RMSE of x / (1 + x) against 1024 spp (tests/test_denoise.py).  For every (radius, gamma)
the table holds the error of the rectified chain beside the two baselines: the plain carried history and a restart without
history.  The chosen row minimises the mean over the cases and frame counts of e_rectified / min(e_plain, e_restart).  The
bounds of test_rectify.test_quality_where_the_history_is_right are the midpoints of 1 and the ratios e_rectified / e_plain on
city-small after 4 and 8 frames at the parameters the cases were stated with (test_rectify.TABLE: radius 2, gamma 1); the
chosen row's ratios are recorded beside them.

    python tools/rectify_quality.py [--out profiles/rectify_quality.json]
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

RADIUS = (1, 2, 3)
GAMMA = (0.5, 0.75, 1.0, 1.25, 1.5, 2.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectify_quality.json"))
    args = ap.parse_args()
    import test_rectify as T
    from yuki_amd import core as yk

    frames = T.QUALITY["frames"]
    base, rows = {}, {}
    for name in T.QUALITY_CASES:
        tparams, films, moved = T.oracle_case(name)
        for radius, gamma in itertools.product(RADIUS, GAMMA):
            e = T.quality_chains(yk, tparams, films, moved, yk.RectifyParams(radius=radius, gamma=gamma))
            for i, k in enumerate(frames):
                base[f"{name}/{k}"] = dict(restart=round(e["restart"][i], 5), plain=round(e["plain"][i], 5))
                best = min(e["plain"][i], e["restart"][i])
                rows.setdefault((radius, gamma), {})[f"{name}/{k}"] = dict(e=round(e["rectified"][i], 5), over_plain=round(e["rectified"][i] / e["plain"][i], 4), over_restart=round(e["rectified"][i] / e["restart"][i], 4), over_best=round(e["rectified"][i] / best, 4))
        print(name, "done", flush=True)
    table = []
    for (radius, gamma), cells in rows.items():
        table.append(dict(radius=radius, gamma=gamma, mean_over_best=round(float(np.mean([c["over_best"] for c in cells.values()])), 4), cells=cells))
    table.sort(key=lambda r: r["mean_over_best"])
    best = table[0]
    stated = next(r for r in table if (r["radius"], r["gamma"]) == (T.TABLE["radius"], T.TABLE["gamma"]))  # what the test asserts at
    ratios = {k: stated["cells"][f"city-small-camera/{k}"]["over_plain"] for k in (4, 8)}
    result = dict(
        what="host instance of yk_history_rectify before every yk_history_blend on oracle films; error = RMSE of x/(1+x) against 1024 spp; a 64-spp history of the state before the change, frames of 4 spp (seeds SEED + 977 k for frame k = 1 ..) after it, max_history 64",
        cases={k: dict(v) for k, v in T.QUALITY_CASES.items()},
        baselines=base,
        chosen=dict(radius=best["radius"], gamma=best["gamma"]),
        asserted_at=dict(T.TABLE),
        city_small_measured_ratio={str(k): v for k, v in ratios.items()},
        city_small_ratio_at_chosen={str(k): best["cells"][f"city-small-camera/{k}"]["over_plain"] for k in (4, 8)},
        city_small_bound={str(k): round((1.0 + v) / 2.0, 4) for k, v in ratios.items()},
        table=table,
    )
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    for r in table:
        print(r["radius"], r["gamma"], r["mean_over_best"])
    print("chosen", result["chosen"], "city-small ratios", ratios, "bounds", result["city_small_bound"])


if __name__ == "__main__":
    main()
