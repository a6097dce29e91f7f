#!/usr/bin/env python3
"""Measure the tolerances of tests/test_guides_through.py::test_restatement_matches_slab_optics.  (CPU only.)

The test compares the independent restatement of the guides-through-glass rule (tests/guides_through_ref.py: oracle
surfaces and lobes, numpy float32 spawn rule and running T) with the float64 closed form of a plane-parallel slab under the
scene's own camera.  How far a correct binary32 walk lands from float64 is measured here, on other rays: the same scene
under the three CALIBRATION_CAMERAS.  The worst error of every figure over them times the margin of
tools/physics_tolerances.py (never below its floor) is the tolerance; the share of slab-path pixels the closed form's own
predicates leave out is recorded beside it and held to the same cap.

The figures go into profiles/physics_tolerances.json beside the others, as the section "guides_through"; nothing else of
that file is read or changed.

    python tools/guides_through_tolerances.py [--out profiles/physics_tolerances.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import guides_through_ref as ref  # noqa: E402
import physics_cases as K  # noqa: E402


def _round(v):
    return float(f"{v:.6g}")


def measure(yk, oracle, log=None):
    worst = {k: 0.0 for k in ref.OPTICS_FIGURES}
    excluded, compared = 0.0, []
    for cam in ref.CALIBRATION_CAMERAS:
        score = ref.slab_score(yk, oracle, cam)
        if log:
            log(f"{cam['position']}: {score}")
        for k in worst:
            worst[k] = max(worst[k], score[k])
        excluded = max(excluded, score["excluded"])
        compared.append(score["compared"])
    assert excluded <= K.MAX_EXCLUDED, excluded
    return dict(
        what="restatement-vs-float64 slab optics under the calibration cameras; tolerance = margin x worst, at least floor (tools/guides_through_tolerances.py)",
        margin=K.MARGIN, floor=K.FLOOR, max_excluded=K.MAX_EXCLUDED, film=list(ref.OPTICS_RES),
        calibration_cameras=[dict(position=list(c["position"]), target=list(c["target"])) for c in ref.CALIBRATION_CAMERAS],
        test_camera=dict(position=list(ref.CAMERA["position"]), target=list(ref.CAMERA["target"])),
        compared=compared,
        rows={k: dict(worst=_round(worst[k]), tolerance=_round(K.adopt(worst[k])), excluded=_round(excluded)) for k in worst},
    )


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=K.TOLERANCES)
    args = ap.parse_args()
    from oracle import binding
    from yuki_amd import core as yk

    binding.lib()
    section = measure(yk, binding, log=lambda s: print(s, file=sys.stderr))
    with open(args.out) as fh:
        whole = json.load(fh)
    whole["guides_through"] = section
    with open(args.out, "w") as fh:
        json.dump(whole, fh, indent=1)
        fh.write("\n")
    print({k: v["tolerance"] for k, v in section["rows"].items()}, "->", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
