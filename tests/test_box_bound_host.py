"""CPU: the box bound of the scene-key kernels' phase 1 (pc_box_bin_range, csrc/ppf_core.h).

tests/native/box_bound_check.c includes the header that the kernels include and checks, for 200 000 seeded random boxes
and points (degenerate boxes, points inside, near and far, five bin widths), that the range of distance bins it gives
holds pc_pair_dist_bin of every tried pair of the point with a point of the box, that the range is no wider than the
box's diagonal plus two bins and the slack, and that it gives none for coordinates that are not finite.  It is built and run twice as
a program of its own: with the library's flags, and under the address and undefined-behaviour sanitizers.  Nothing is
loaded into Python and no call reaches a device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "objective-slam_amd", "csrc")
COMMON = ["gcc", "-g", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
          os.path.join(ROOT, "tests", "native", "box_bound_check.c")]


@pytest.mark.parametrize("name,flags", [
    ("box_bound_check", ["-O2"]),                                   # csrc/Makefile's CFLAGS
    ("box_bound_check_san", ["-O1", "-fsanitize=address,undefined", "-static-libasan", "-fno-sanitize-recover=all"]),
])
def test_box_range_holds_every_pair_of_the_box(name, flags):
    out = os.path.join(ROOT, "build", name)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(COMMON + flags + ["-lm", "-o", out], check=True)
    r = subprocess.run([out], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b"box_bound_check ok" in r.stdout, (r.returncode, r.stderr.decode()[-2000:])
