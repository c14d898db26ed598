"""The order in which tests/test_gpu_decode_session.py lets the decoder's entry points meet on one session
(tests/decode_session.py: schedule and the two short forms).  Pure Python: no device, no library."""
import itertools

import pytest

import decode_session as ds


def test_the_schedule_of_the_nine_operations_covers_every_ordered_pair():
  assert len(ds.OPS) == 9 and len(set(ds.OPS)) == 9
  seq = ds.schedule(ds.OPS)
  assert len(seq) == 82
  assert set(seq) == set(ds.OPS)
  every = set(itertools.product(ds.OPS, repeat=2))
  assert len(every) == 81 and ds.pairs_of(seq) == every
  # 81 edges in 81 adjacent positions: every pair exactly once, an Eulerian circuit and not a walk that happens to cover
  adjacent = list(zip(seq[:-1], seq[1:]))
  assert len(adjacent) == 81 and len(set(adjacent)) == 81
  assert seq[0] == seq[-1] == ds.OPS[0]


def test_the_schedule_is_the_same_list_on_every_call():
  first = ds.schedule(ds.OPS)
  for _ in range(3):
    assert ds.schedule(ds.OPS) == first
  assert ds.schedule(list(ds.OPS)) == first and ds.schedule(iter(ds.OPS)) == first


@pytest.mark.parametrize("first", ds.OPS)
def test_the_schedule_begins_with_the_operation_passed_first(first):
  ops = [first] + [o for o in ds.OPS if o != first]
  seq = ds.schedule(ops)
  assert seq[0] == first and len(seq) == 82
  assert ds.pairs_of(seq) == set(itertools.product(ds.OPS, repeat=2))


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_other_sizes(n):
  ops = list(range(n))
  seq = ds.schedule(ops)
  assert len(seq) == n * n + 1 and ds.pairs_of(seq) == set(itertools.product(ops, repeat=2))
  assert ds.schedule([]) == []
  with pytest.raises(ValueError):
    ds.schedule(["P", "P"])


def test_the_short_schedules():
  seq = ds.around("P", ds.OPS)
  assert len(seq) == 17 and seq[0] == seq[-1] == "P"
  others = [o for o in ds.OPS if o != "P"]
  assert ds.pairs_of(seq) == {("P", o) for o in others} | {(o, "P") for o in others}
  for first in ("P", "L", "V6", "C", "S", "X"):
    seq = ds.hand_over(first, ds.OPS)
    assert seq[0] == first and seq[-3:] == ["P", "L", "C"] and len(seq) == 12
    assert sorted(seq[:9]) == sorted(ds.OPS)
