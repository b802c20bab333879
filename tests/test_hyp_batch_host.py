"""The host part of csrc/hyp_batch.hpp without a device: builds
tests/hyp_batch_host.cpp host-only under AddressSanitizer and
UndefinedBehaviorSanitizer and runs it, as tests/test_staging.py does for
staging.hpp.  The program holds the assertions: the block table against the
closed-form rule it replaces (either side of one and of four LDS tiles, dead
rows between live ones, no live row, the launch limit), the runs of live rows
the download loop visits, the sample-table check with its messages, and the
inverse of K_REF.
"""
import os
import subprocess

import pytest

from conftest import PKG, REPO

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hyp_batch") / "hyp_batch_host")
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-x", "c++", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-I" + os.path.join(PKG, "csrc"), "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(REPO, "tests", "hyp_batch_host.cpp"), "-o", exe,
           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def test_host_helpers_match_the_code_they_replace(program):
    r = subprocess.run([program], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    assert r.stderr == "", r.stderr  # no sanitizer report
