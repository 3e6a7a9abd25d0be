"""The scalar SGBM rules (csrc/sdr_sgbm_rules.hpp) on the host: tests/cpp/sgbm_rules_check.hip built
as a plain host program (no sanitizer flags; the sanitizer build is run by hand, see its header) and
run once."""
import os
import subprocess

from stereo_depth_ruler_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sgbm_rules_check_host_program(tmp_path):
    exe = str(tmp_path / "sgbm_rules_check")
    subprocess.check_call([B._hipcc(), "--cuda-host-only", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "sgbm_rules_check.hip"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("sgbm_rules_check: ") and last.endswith(" checks, 0 failures"), last
