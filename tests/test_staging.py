"""csrc/staging.hpp's packed-buffer arithmetic without a device: builds
tests/staging_layout.cpp host-only under AddressSanitizer and
UndefinedBehaviorSanitizer and runs it.  The program holds the assertions
(256-byte slots, empty slots, the offsets and totals of the three CSR entry
points against the closed-form chains they replace); a device pointer asked
for before reserve() must end the program.
"""
import os
import subprocess

import pytest

from conftest import PKG, REPO

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("staging") / "staging_layout")
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-x", "c++", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-I" + os.path.join(PKG, "csrc"), "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(REPO, "tests", "staging_layout.cpp"), "-o", exe,
           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def test_layout_matches_the_closed_form_chains(program):
    r = subprocess.run([program], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    assert r.stderr == "", r.stderr  # no sanitizer report


def test_device_pointer_before_reserve_is_rejected(program):
    r = subprocess.run([program, "early-ptr"], capture_output=True, text=True)
    assert r.returncode != 0 and "device pointer before reserve()" in r.stderr, (r.returncode, r.stdout, r.stderr)
    assert r.stdout == ""  # no pointer was handed out
