"""The plan of a scene change (yuki_amd/csrc/yk_scene_change.h): which route yk_scene_update[_device] and
yk_scene_apply_edit[_device] ask for, what goes up for staging, which tables, boxes and records are rewritten, what follows
a device step that failed and which reason is reported — pure functions over plain values, checked against the table written
by hand in tests/cpp/scene_change_table.inc (tests/cpp/scene_change_plan_test.cpp).  The header includes no HIP, so a plain
host compile builds the test.  ROWS is that table for the tests that hold the library itself to it."""
import os
import re
import subprocess
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")

Row = namedtuple("Row", "scene brings has_spheres kinds_changed verdict device_plan upload spheres kind_tables boxes records")


def read_rows():
    """scene_change_table.inc as Row tuples: names as strings, the flags as ints."""
    rows = []
    with open(os.path.join(CPP, "scene_change_table.inc")) as f:
        for line in f:
            m = re.match(r"ROW\((.*)\)\s*$", line)
            if m:
                cells = [c.strip() for c in m.group(1).split(",")]
                rows.append(Row(*[int(c) if c.isdigit() else c for c in cells]))
    return rows


ROWS = read_rows()


def row_of(scene, brings, has_spheres, kinds_changed):
    (row,) = [r for r in ROWS if (r.scene, r.brings, r.has_spheres, r.kinds_changed) == (scene, brings, int(bool(has_spheres)), int(bool(kinds_changed)))]
    return row


def test_scene_change_plan(tmp_path):
    exe = str(tmp_path / "scene_change_plan_test")
    subprocess.check_call(["hipcc", "-x", "c++", "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(CPP, "scene_change_plan_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "scene_change_plan_test: ok" in out.stdout, out.stdout + out.stderr


def test_the_table_reads_as_the_program_reads_it():
    assert len(ROWS) == 48 and len({r[:4] for r in ROWS}) == 48
    assert {r.scene for r in ROWS} == {"HOST_ONLY", "HOST_LAID", "DEVICE_LAID"} and {r.verdict for r in ROWS} == {"REFUSED", "HOST", "DEVICE"}
    assert row_of("DEVICE_LAID", "SPHERES_HOST", True, False) == Row("DEVICE_LAID", "SPHERES_HOST", 1, 0, "DEVICE", 1, 1, 1, 1, 1, 1)
