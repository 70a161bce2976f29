"""CPU: the host stages' shared arithmetic (csrc/oslam_rigid.h) against the expressions it replaced, bit for bit.

tests/native/rigid_check.c includes the header alone, carries the earlier expressions as literal copies and compares
with memcmp over the identity, 10 000 random poses, rotations at the edge of the orthonormality tolerance, translations
with -0.0f and denormals, the all-zero test's edge values and clouds of 1, 2, 3 and 1501 points.  It is built and run
twice as a program of its own: with the library's floating-point flags, and under the address and undefined-behaviour
sanitizers.  Nothing is loaded into Python and no call reaches a device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "objective-slam_amd", "csrc")
COMMON = ["gcc", "-g", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
          os.path.join(ROOT, "tests", "native", "rigid_check.c")]


@pytest.mark.parametrize("name,flags", [
    ("rigid_check", ["-O2"]),                                       # csrc/Makefile's CFLAGS
    ("rigid_check_san", ["-O1", "-fsanitize=address,undefined", "-static-libasan", "-fno-sanitize-recover=all"]),
])
def test_rigid_header_keeps_the_bits(name, flags):
    out = os.path.join(ROOT, "build", name)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(COMMON + flags + ["-o", out, "-lm"], check=True)
    r = subprocess.run([out], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b"rigid_check ok" in r.stdout, (r.returncode, r.stderr.decode()[-2000:])
