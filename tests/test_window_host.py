"""CPU: the shifting window's arithmetic (csrc/oslam_window.h) against brute force and against the expressions it replaced.

tests/native/window_check.c includes the header alone.  The entering region of a shift is held to a voxel-by-voxel count
for a ragged 5 x 3 x 4 window at three offsets under every shift of -6..6 x -4..4 x -5..5, and to volumes and interval
tests at 256^3 and at offsets of +-(2^20 - 8); the origin of an offset, the global coordinate of a linear index and back,
and the bricks a window overlaps are compared with literal copies of the earlier code (the origin with memcmp, -0.0f and a
denormal among the inputs); the layout of a batch of records is computed in size_t up to 2^31 - 1 records.  It is built
and run twice as a program of its own: with the library's floating-point flags, and under the address and
undefined-behaviour sanitizers.  Nothing is loaded into Python and no call reaches a device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "objective-slam_amd", "csrc")
COMMON = ["gcc", "-g", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
          os.path.join(ROOT, "tests", "native", "window_check.c")]


@pytest.mark.parametrize("name,flags", [
    ("window_check", ["-O2"]),                                      # csrc/Makefile's CFLAGS
    ("window_check_san", ["-O1", "-fsanitize=address,undefined", "-static-libasan", "-fno-sanitize-recover=all"]),
])
def test_window_header_keeps_the_rules(name, flags):
    out = os.path.join(ROOT, "build", name)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(COMMON + flags + ["-o", out], check=True)
    r = subprocess.run([out], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b"window_check ok" in r.stdout, (r.returncode, r.stderr.decode()[-2000:])
