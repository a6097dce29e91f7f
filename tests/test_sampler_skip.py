"""sampler_skip_2d (yuki_amd/csrc/yk_rng.h): the state transition of sampler_get_2d without its values — what the light loops
call for a light that does not read its sample.  Both sampler kinds, Stratified 2x2 and 8x8 with jitter on and off: the whole
SamplerState and the next three draws equal those after a real draw (tests/cpp/sampler_skip_test.cpp).  The samplers are
__host__ __device__, so a host-only compile of the header builds the test."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sampler_skip_matches_draw(tmp_path):
    exe = str(tmp_path / "sampler_skip_test")
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "sampler_skip_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "sampler_skip_test: ok" in out.stdout, out.stdout + out.stderr
