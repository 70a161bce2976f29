"""CPU: the batch plan of a registration (csrc/oslam_vote_plan.h) against the walk it replaced.

tests/native/vote_plan_check.c includes the header alone, carries the earlier batch rule and its walk as literal copies
and compares, per batch, first reference point, size, slots and all the offsets: no and one reference point, all-zero,
odd and even demands, demands at the limit and one place either side of it after rounding, a reference point larger
than the limit, a running total that reaches the 32-bit bound before the limit, and 10 000 seeded random demand vectors
against small limits.  Every plan tiles the reference points in order, has even offsets and exceeds the limit only with
a batch of one.  It is built and run twice as a program of its own: with the library's flags, and under the address and
undefined-behaviour sanitizers.  Nothing is loaded into Python and no call reaches a device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "objective-slam_amd", "csrc")
COMMON = ["gcc", "-g", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
          os.path.join(ROOT, "tests", "native", "vote_plan_check.c")]


@pytest.mark.parametrize("name,flags", [
    ("vote_plan_check", ["-O2"]),                                   # csrc/Makefile's CFLAGS
    ("vote_plan_check_san", ["-O1", "-fsanitize=address,undefined", "-static-libasan", "-fno-sanitize-recover=all"]),
])
def test_vote_plan_equals_the_walk_it_replaced(name, flags):
    out = os.path.join(ROOT, "build", name)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(COMMON + flags + ["-o", out], check=True)
    r = subprocess.run([out], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b"vote_plan_check ok" in r.stdout, (r.returncode, r.stderr.decode()[-2000:])
