#!/usr/bin/env python3
"""Measure the tolerances of the physics tests.  (CPU only.)

tests/test_physics.py (oracle) and tests/test_gpu_physics.py (device) compare shading with the float64 physics of
tests/physics_ref.py; how far a correct f32 implementation lands from float64 is measured here, not guessed.  For every
deterministic case of tests/physics_cases.py this script runs the CPU oracle on the case's CALIBRATION seeds (disjoint
from the seeds the tests use; a seed fixes the camera pose and tiles, the rays' places and headings or the sampler's stream), takes the worst error of every figure over them and adopts 4 x that as the tolerance (never
below one f32 ulp): the margin covers the seed-to-seed spread of f32 rounding, while a misread term shows at 1e-3 or more
(the tests' power check).  It records beside each tolerance the share of rows that the case's input predicates excluded.

For the Monte-Carlo cases (Uniform sampler, fixed seed) it finds N, the smallest power of two from 256 whose relative
standard error on the oracle is at most 1 %, capped at 65,536, and records the z value |mean - truth| / standard error the
oracle reaches there.  The run is deterministic, and the device equals the oracle bit for bit, so nothing is calibrated
on the device.  A |z| above 3 needs the `notes` entry below to say why it is chance, or another sampler seed.

    python tools/physics_tolerances.py [--out profiles/physics_tolerances.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import physics_cases as K  # noqa: E402

NOTES = {}  # Monte-Carlo case -> why a |z| > 3 on the oracle is chance and not bias (none needed so far)


def _round(v):
    return float(f"{v:.6g}")


def measure_row(be, case_id):
    """{figure: dict(worst, tolerance, excluded)} of one deterministic case over its calibration seeds."""
    _, _, _, calibration = K.all_cases()[case_id]
    worst, excluded = {}, {}
    for seed in calibration:
        score = K.run_case(be, case_id, seed, cache=False)
        for k, v in score.items():
            if K.is_toleranced(k):
                worst[k] = max(worst.get(k, 0.0), v)
                share = score.get(k[:2] + "excluded", score.get("excluded", 0.0))  # statistical figures (`_z`) are held to Z_MAX, not calibrated
                excluded[k] = max(excluded.get(k, 0.0), share)
    return {k: dict(worst=_round(worst[k]), tolerance=_round(K.adopt(worst[k])), excluded=_round(excluded[k])) for k in worst}


def measure_mc(be, name):
    spec = K.mc_cases()[name]
    truth = K.mc_truth(spec)
    n = 256
    while True:
        fig = K.mc_figures(K.mc_samples(be, spec, n), truth)
        if fig["rel_se"] <= 0.01 or n >= 65536:
            break
        n *= 2
    out = dict(n=n, rel_se=_round(fig["rel_se"]), z=_round(fig["z"]), mean=_round(fig["mean"]), truth=_round(fig["truth"]))
    if name == "floor-under-pane":  # its truth is that of infinite plates and unbounded depth: the bound on what that leaves out
        out["bias_bound"] = _round(K.under_pane_bias())
        assert out["bias_bound"] <= 0.1 * out["rel_se"], "widen the plates"
    if name in NOTES:
        out["note"] = NOTES[name]
    return out


def measure(be, log=None):
    rows = {}
    for case_id in K.all_cases():
        for k, v in measure_row(be, case_id).items():
            rows[f"{case_id}:{k}"] = v
        if log:
            log(case_id)
    mc = {}
    for name in K.mc_cases():
        mc[name] = measure_mc(be, name)
        if log:
            log(f"{name}: N {mc[name]['n']}, z {mc[name]['z']}")
    return dict(
        what="oracle-vs-float64 errors on calibration seeds; tolerance = margin x worst, at least floor (tools/physics_tolerances.py)",
        margin=K.MARGIN, floor=K.FLOOR, max_excluded=K.MAX_EXCLUDED,
        calibration_seeds=dict(bsdf=list(K.BSDF_CALIBRATION), light=list(K.LIGHT_CALIBRATION), li=list(K.LI_CALIBRATION), sampler=[K.MC_SEED + 1, K.MC_SEED + 2],
                               camera=list(K.CAMERA_CALIBRATION), whitted=list(K.WHITTED_CALIBRATION), surface=list(K.SURFACE_CALIBRATION)),
        test_seeds=dict(bsdf=[K.BSDF_SEED, K.BSDF_SEED + 1], light=K.LIGHT_SEEDS, li=K.LI_SEED, sampler=K.MC_SEED, camera=K.CAMERA_SEED, whitted=K.WHITTED_SEED, surface=K.SURFACE_SEED),
        rows=rows, monte_carlo=mc,
    )


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=K.TOLERANCES)
    args = ap.parse_args()
    from oracle import binding

    binding.lib()
    result = measure(K.OracleBackend(binding), log=lambda s: print(s, file=sys.stderr))
    beyond = [k for k, v in result["monte_carlo"].items() if abs(v["z"]) > 3 and "note" not in v]
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(f"{len(result['rows'])} tolerances and {len(result['monte_carlo'])} Monte-Carlo cases -> {args.out}")
    if beyond:
        print("z beyond 3 without a note:", beyond)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
