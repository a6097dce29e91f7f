"""300 seeded random Mitsuba files (tools/mitsuba_fuzz.py: valid files with dropped / duplicated / reordered attributes and
children, respelled numbers, nested ignored subtrees, renamed elements, and the three kinds of malformed XML the loader
keeps the reference's behaviour for): yk_load_mitsuba and tests/mitsuba_ref.py both accept a file and agree bit for bit in
every field, or both reject it."""
import os
import sys

import pytest

from yuki_amd import loaders
from yuki_amd._ffi import YukiError

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import mitsuba_fuzz  # noqa: E402

SEEDS = list(range(300))  # frozen: the checker alone accepts 147 of them (tools/mitsuba_fuzz.py --rate 300)


def test_fuzzed_files_load_alike_or_are_rejected_by_both(tmp_path, oracle):
    import mitsuba_ref as mr

    accepted, kinds = 0, {}
    for seed in SEEDS:
        p, done = mitsuba_fuzz.write_case(str(tmp_path), seed)
        try:
            want = mr.load_mitsuba(p)
        except mr.LoadError as e:
            want = None
            with pytest.raises(YukiError):
                loaders.load_mitsuba(p)
                pytest.fail(f"seed {seed} {done}: the checker rejects it ({e}), the library loads it")
        if want is not None:
            try:
                got = loaders.load_mitsuba(p)
            except YukiError as e:
                pytest.fail(f"seed {seed} {done}: the checker loads it, the library rejects it ({e})")
            try:
                mr.assert_same_loaded(want, got)
            except AssertionError as e:
                raise AssertionError(f"seed {seed} {done}: {e}") from e
            accepted += 1
        for k in done or ["none"]:
            kinds[k] = kinds.get(k, 0) + 1
    print(f"{accepted} of {len(SEEDS)} files accepted by both; mutations applied: {sorted(kinds.items())}")
    # a run that rejects most files proves nothing about values: at least 40 % must be accepted by the checker alone
    assert accepted >= 0.4 * len(SEEDS), accepted
    assert len(kinds) >= 12  # every kind of mutation occurs among the seeds
