"""csrc/extract_plan.hpp's host arithmetic without a device: builds
tests/extract_plan_check.cpp host-only under AddressSanitizer and
UndefinedBehaviorSanitizer and runs it.  The program holds the assertions
(octave sizes and offsets, the taps, the candidate bound, the chunk size, the
candidate key's order).
"""
import os
import subprocess

from conftest import PKG, REPO

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_plan_arithmetic_holds_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "extract_plan_check")
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-x", "c++", "-I" + os.path.join(PKG, "csrc"),
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(REPO, "tests", "extract_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    assert r.stderr == "", r.stderr  # no sanitizer report
