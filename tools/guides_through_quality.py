#!/usr/bin/env python3
"""Measure what guides through glass buy the denoiser, on oracle-rendered films.  (CPU only.)

For each quality scene of tests/guides_through_ref.py (the slab scene at 64 x 36, the Cornell box at 48 x 48): a 4-spp film
against a 1024-spp film, the host denoiser with default DenoiseParams, steered once by first-hit guides and once by the
restatement's through-guides; on every scene also the demodulated filter with the albedo of each pass's own ids.  The
error is test_denoise.quality_error over the pixels seen through glass (through >= 1 and hit); the figure is the ratio
through / first-hit, below 1 where the pass gains.  Measured on three sampler seeds, none of them the test's; the test
asserts, on its own seed, a ratio <= the midpoint between the worst measured ratio and 1 — and nothing for a figure whose
worst measured ratio is >= 0.95: there the pass gains nothing worth holding, and README says so.  The whole-film ratio is
reported, never asserted.

    python tools/guides_through_quality.py [--out profiles/guides_through_quality.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import guides_through_ref as ref  # noqa: E402

NO_GAIN = 0.95
RATIOS = ("ratio", "film_ratio", "albedo_ratio", "albedo_film_ratio")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guides_through_quality.json"))
    args = ap.parse_args()
    from oracle import binding as oracle
    from yuki_amd import core as yk

    oracle.lib()
    result = dict(
        tool="tools/guides_through_quality.py",
        what="masked quality_error of the host denoiser (default DenoiseParams) under through-guides over the same under first-hit guides; mask = through >= 1 and hit",
        settings={k: (hex(v) if k.endswith("seed") else v) for k, v in ref.QUALITY.items()},
        calibration_seeds=[hex(s) for s in ref.QUALITY_CALIBRATION_SEEDS], test_seed=hex(ref.QUALITY_TEST_SEED), no_gain_at=NO_GAIN, scenes={},
    )
    for name, res in ref.QUALITY_SCENES.items():
        runs = {hex(seed): ref.quality_figures(yk, oracle, name, seed) for seed in ref.QUALITY_CALIBRATION_SEEDS}
        worst = {k: max(r[k] for r in runs.values()) for k in RATIOS}
        asserted = {k: (None if worst[k] >= NO_GAIN else 0.5 * (worst[k] + 1.0)) for k in ("ratio", "albedo_ratio")}
        result["scenes"][name] = dict(film=list(res), masked_pixels=next(iter(runs.values()))["masked_pixels"], runs={s: {k: round(v, 5) if isinstance(v, float) else v for k, v in r.items()} for s, r in runs.items()},
                                      worst={k: round(v, 5) for k, v in worst.items()}, asserted={k: (None if v is None else round(v, 5)) for k, v in asserted.items()})
        print(name, "worst:", result["scenes"][name]["worst"], "asserted:", result["scenes"][name]["asserted"], file=sys.stderr)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("->", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
