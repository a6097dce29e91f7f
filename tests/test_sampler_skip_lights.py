"""The light loop of a vertex under lights that ignore their sample (light_draw_2d, yuki_amd/csrc/yk_shade.h) calls
sampler_skip_2d once per light.  n skips against n real draws for all three samplers of the GPU tests and the flagship's
8x8, at every dimension a depth-8 path with 1 to 4 lights reaches, with the BSDF and roulette draws that follow
(tests/cpp/sampler_skip_lights_test.cpp).  Host only: the samplers are __host__ __device__."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_light_loop_of_skips_matches_draws(tmp_path):
    exe = str(tmp_path / "sampler_skip_lights_test")
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "sampler_skip_lights_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "sampler_skip_lights_test: ok" in out.stdout, out.stdout + out.stderr
