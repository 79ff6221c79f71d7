"""The generator of the interleaved call sequence (tests/call_sequence.py): every ordered pair of different configurations occurs,
the sequence is as short as that allows, and a seed fixes it."""
import pytest

from tests import call_sequence as cs

NAMES = ["A", "B", "C", "D", "E", "F", "F'", "G", "H"]       # the configurations of tests/test_call_sequence_gpu.py


@pytest.mark.parametrize("names", [NAMES, ["x", "y"], list(range(5))])
@pytest.mark.parametrize("seed", [0, 1, 20240])
def test_every_ordered_pair_occurs_exactly_once(names, seed):
    seq = cs.sequence(names, seed)
    n = len(names)
    assert len(seq) == n * (n - 1) + 1 and seq[0] == seq[-1]
    pairs = list(zip(seq[:-1], seq[1:]))
    assert len(set(pairs)) == len(pairs) == n * (n - 1)
    assert set(pairs) == {(x, y) for x in names for y in names if x != y}
    assert cs.covers_every_ordered_pair(seq, names)


def test_the_sequence_is_fixed_by_its_seed_and_differs_between_seeds():
    assert cs.sequence(NAMES, 3) == cs.sequence(NAMES, 3)
    assert cs.sequence(NAMES, 3) != cs.sequence(NAMES, 4)


def test_the_coverage_check_notices_a_missing_pair_and_a_repeat():
    seq = cs.sequence(NAMES, 0)
    assert not cs.covers_every_ordered_pair(seq[:-1], NAMES)
    assert not cs.covers_every_ordered_pair(seq + [seq[-1]], NAMES)
