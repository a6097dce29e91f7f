"""The plan of a render submission (yuki_amd/csrc/yk_render_plan.h): tiles -> pixel offsets, the accumulating film's rules, the
chunks under sample_buf_cap, the batch, the HBM clamp and the work sets — pure functions over plain numbers, checked on cases
worked out by hand (tests/cpp/render_plan_test.cpp).  The header includes no HIP, so a plain host compile builds the test."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_render_plan_arithmetic(tmp_path):
    exe = str(tmp_path / "render_plan_test")
    subprocess.check_call(["hipcc", "-x", "c++", "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "render_plan_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "render_plan_test: ok" in out.stdout, out.stdout + out.stderr
