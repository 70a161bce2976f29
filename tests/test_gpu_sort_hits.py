"""GPU: k_sort_hits alone, through oslam_sort_hits_tap, on every case of tests/sort_inputs.py.

The five arrays the tap copies back -- the sorted key words with their marker bit, the two payload words, the runs and
the run counts -- equal the restatement (tests/sort_ref.py) word for word, the words the kernel does not own included:
the tap fills them with 0xA5 bytes before the launch and the restatement expects them back.  Integers only: no
tolerance.  tests/test_sort_host.py proves on the CPU that every case reaches the edge it is named for."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sort_inputs as I  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("key words", "theta", "idx", "runs", "run counts")


def _first_difference(got, want):
    at = np.argwhere(got != want)
    return None if len(at) == 0 else (tuple(at[0].tolist()), hex(int(got[tuple(at[0])])), hex(int(want[tuple(at[0])])))


@pytest.mark.parametrize("name", sorted(I.CASES))
def test_sort_equals_the_restatement(ppf, name):
    bits, (num, th, idx, off, cnt), want, _, _ = I.reference(name)
    got = ppf.sort_hits(num, th, idx, off, cnt, bits)
    for what, g, w in zip(NAMES, got, want[:5]):
        assert g.shape == w.shape and g.dtype == w.dtype, what
        assert np.array_equal(g, w), (name, what, "first difference (place, got, want)", _first_difference(g, w))


def test_sort_is_the_same_twice(ppf):
    """the same launch again: the order among equal keys comes from arrival, not from which wave got there first"""
    bits, (num, th, idx, off, cnt), want, _, _ = I.reference("lengths_around_two_segments")
    first = ppf.sort_hits(num, th, idx, off, cnt, bits)
    again = ppf.sort_hits(num, th, idx, off, cnt, bits)
    assert all(np.array_equal(a, b) and np.array_equal(a, w) for a, b, w in zip(first, again, want[:5]))
