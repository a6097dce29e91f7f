"""The plan of a pixel-list render (yuki_amd/csrc/yk_render_plan.h, RenderPlan::set_pixel_list): chunks cut by pixel count
under sample_buf_cap that cover the list exactly once, and the refusals — checked on cases worked out by hand
(tests/cpp/pixel_list_plan_test.cpp).  The header includes no HIP, so a plain host compile builds the test."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pixel_list_plan_arithmetic(tmp_path):
    exe = str(tmp_path / "pixel_list_plan_test")
    subprocess.check_call(["hipcc", "-x", "c++", "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "pixel_list_plan_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "pixel_list_plan_test: ok" in out.stdout, out.stdout + out.stderr
