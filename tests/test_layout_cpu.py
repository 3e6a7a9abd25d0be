"""The scratch layout rule (csrc/sdr_layout.hpp: typed slices, each 256-byte aligned) on the host:
tests/cpp/layout_check.hip built as a stand-alone host program under the address and
undefined-behaviour sanitizers and run once.  No device is used."""
import os
import subprocess

from stereo_depth_ruler_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = [x for f in ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined") for x in ("-Xarch_host", f)]


def test_layout_check_host_program(tmp_path):
    exe = str(tmp_path / "layout_check")
    subprocess.check_call([B._hipcc(), "--cuda-host-only", "-O1", "-g", "-std=c++17", *SANITIZE,
                           os.path.join(ROOT, "tests", "cpp", "layout_check.hip"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    # a sanitizer report ends the program with a status of its own and text on stderr
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("layout_check: ") and last.endswith(" checks, 0 failures"), last
