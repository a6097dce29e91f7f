#!/usr/bin/env python3
"""Measure the tolerance of the sphere case of the motion pass.  (CPU only.)

tests/test_scene_edit.py compares the host instance of yk_surface_motion_spheres with the float64 statement of a sphere
point's previous position (tests/scene_edit_ref.py) on a 24 x 24 view of glass_balls whose spheres were translated and
rotated; the device instance equals the host one bit for bit, and the chain test of tests/test_gpu_scene_edit.py holds the
reprojected history to the same figure.  How far a correct float32 implementation lands from float64 is measured here on
the CALIBRATION seeds (disjoint from the seed the test uses; a seed fixes every sphere's move): the worst error over them,
in scene diagonals, times 4 — the margin tools/physics_tolerances.py uses for differences that are rounding only.

    python tools/scene_edit_tolerances.py [--out profiles/scene_edit_tolerances.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_scene_edit as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_edit_tolerances.json"))
    args = ap.parse_args()
    from oracle import binding as oracle
    from yuki_amd import core as yk

    rows = []
    for seed in T.CALIBRATION_SEEDS:
        err, n = T.motion_error(yk, oracle, seed)
        rows.append(dict(seed=seed, error=float(f"{err:.6g}"), sphere_pixels=n))
        print(rows[-1])
    worst = max(r["error"] for r in rows)
    out = {
        "what": "yk_surface_motion_spheres, host instance, against the float64 statement: largest |p_prev - p_prev64| over the sphere pixels of a 24 x 24 glass_balls view, in scene diagonals",
        "script": "tools/scene_edit_tolerances.py",
        "margin": 4,
        "sphere_motion_p_prev": dict(worst=worst, tolerance=float(f"{4 * worst:.6g}"), seeds=list(T.CALIBRATION_SEEDS), rows=rows),
    }
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
