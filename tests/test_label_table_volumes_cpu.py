"""Pins the constructions of tests/label_table_volumes.py on the CPU: for every case that tests/test_gpu_label_table.py
runs through the kernels, the port's own stream must state exactly the N (components), U (labels), key width and L
(label section bytes) that the case claims, name every component's label as the construction orders them, and decode
back to the volume.  A case that drifts off its edge fails here, before any GPU time is spent."""
import numpy as np
import pytest

import crackle_amd
import label_table_volumes as ltv


def _pin(case, port):
  arr = case.volume()
  assert arr.shape == case.shape and arr.dtype == case.dtype and arr.flags.f_contiguous
  stream = port.compress(arr, markov_model_order=case.markov)
  assert ltv.read_claims(stream) == case.claims, case.id
  head = crackle_amd.header(stream)
  assert head.stored_data_width == case.stored_width and head.markov_model_order == case.markov
  want = ltv.component_labels(case.shape, case.n, case.values, case.dtype)
  assert np.array_equal(ltv.read_component_labels(stream), want), case.id
  assert np.array_equal(np.unique(want), np.sort(case.values))
  back = port.decompress(stream).reshape(arr.shape, order="F")
  assert back.dtype == arr.dtype and np.array_equal(back, arr)
  return stream, want


def _ids(cases):
  return [c.id for c in cases]


def test_components_volume_counts_what_it_says():
  """The construction against a plain union-find count, without any codec."""
  for shape, n, values in (((7, 5, 3), 40, [9, 1, 2, 3]), ((5, 4, 2), 40, [1, 2, 3]), ((4, 1, 1), 4, [3, 1, 2]), ((2, 1, 5), 10, [8, 9]),
                           ((1, 1, 6), 6, [4]), ((1, 9, 2), 11, [0, 5, 6]), ((9, 8, 4), 13, [7, 200, 90])):
    arr = ltv.components_volume(shape, n, np.array(values, dtype=np.uint64), np.uint8)
    assert ltv.count_components(arr) == n, (shape, n)
    assert sorted(np.unique(arr).tolist()) == sorted(values)
    per = [ltv.count_components(arr[:, :, z:z + 1]) for z in range(shape[2])]
    assert max(per) - min(per) <= 1 and sum(per) == n


def test_components_volume_refuses_what_would_merge():
  u8 = np.uint8
  with pytest.raises(ValueError):      # sx a multiple of the cycle: (128, ., .) with four cycling labels collapses
    ltv.components_volume((128, 4, 1), 300, np.array([9, 1, 2, 3, 4], dtype=np.uint64), u8)
  ltv.components_volume((128, 4, 1), 100, np.array([9, 1, 2, 3, 4], dtype=np.uint64), u8)      # one row of single pixels: nothing above them
  with pytest.raises(ValueError):      # two single pixels side by side, one label for them
    ltv.components_volume((4, 1, 1), 3, np.array([1, 2], dtype=np.uint64), u8)
  with pytest.raises(ValueError):      # fewer single pixels than labels to show
    ltv.components_volume((9, 8, 1), 3, np.array([1, 2, 3, 4], dtype=np.uint64), u8)
  with pytest.raises(ValueError):      # more components than pixels, fewer than slices
    ltv.components_volume((2, 2, 2), 9, np.array([1, 2, 3], dtype=np.uint64), u8)
  with pytest.raises(ValueError):
    ltv.components_volume((2, 2, 2), 1, np.array([1], dtype=np.uint64), u8)
  with pytest.raises(ValueError):      # equal values, a value beyond the dtype
    ltv.components_volume((9, 8, 1), 9, np.array([1, 2, 2], dtype=np.uint64), u8)
  with pytest.raises(ValueError):
    ltv.components_volume((9, 8, 1), 9, np.array([1, 2, 300], dtype=np.uint64), u8)


def test_value_sets():
  for u in (3, 2049, 65537):
    for order in ltv.ORDERS.values():
      v = order(u, 10, 3)
      assert v.dtype == np.uint64 and np.array_equal(np.sort(v), 10 + 3 * np.arange(u, dtype=np.uint64))
  p = ltv.permuted(4097)
  assert not np.all(np.diff(p.astype(np.int64)) > 0) and not np.all(np.diff(p.astype(np.int64)) < 0)
  lo = ltv.low32_equal(3001)
  assert np.all(lo & np.uint64(0xFFFFFFFF) == 5) and np.unique(lo).size == 3001 and int(lo[1]) == (1 << 33) | 5
  assert int(ltv.dense(5)[0]) == 0 and np.all(ltv.pow2_multiples(9, 40) & np.uint64((1 << 40) - 1) == 0)
  assert np.array_equal(ltv.by_appearance(np.array([1, 2, 3], dtype=np.uint64)), [3, 1, 2])


HASH = ltv.hash_threshold_cases()


@pytest.mark.parametrize("case", HASH, ids=_ids(HASH))
def test_hash_threshold_cases(case, port):
  _pin(case, port)


def test_hash_threshold_cases_sit_on_the_table_sizes():
  ns = sorted({c.n for c in HASH})
  assert ns == [8192, 8193, 16384, 16385, 32768, 32769]
  assert [n > ltv.HASH_ABOVE for n in ns] == [False, True, True, True, True, True]
  assert [ltv.hash_slots(n) for n in ns[1:]] == [32768, 32768, 65536, 65536, 131072]
  full = [c for c in HASH if c.u == c.n]
  assert sorted(2 * c.u == ltv.hash_slots(c.n) for c in full) == [False, False, True, True]      # exactly half full, and just past the step


SORT = ltv.sort_size_cases()


@pytest.mark.parametrize("case", SORT, ids=_ids(SORT))
def test_sort_size_cases(case, port):
  assert case.n > ltv.HASH_ABOVE      # the hash pass runs: the network sorts the U distinct labels
  _pin(case, port)


def test_sort_size_cases_reach_every_kernel_mix():
  pads = sorted({ltv.padded_sort_size(c.u) for c in SORT})
  assert pads == [2048, 4096, 8192, 16384, 32768, 131072, 262144]
  for u in (2048, 2049, 4096, 4097, 8192, 8193, 16385, 65537, 1 << 18):
    assert sorted(c.id.rsplit("-", 1)[1] for c in SORT if c.u == u) == ["asc", "desc", "perm"]
  # the global steps of the last stage k = n_pad: distances n_pad / 2 down to 2048, taken two at a time while >= 4096
  steps = {p: len([j for j in (p >> s for s in range(1, 20)) if j >= 2048]) for p in pads}
  assert {steps[p] % 2 for p in pads if p >= 16384} == {0, 1}


SORT_ALL = ltv.sort_all_cases()


@pytest.mark.parametrize("case", SORT_ALL, ids=_ids(SORT_ALL))
def test_sort_all_cases(case, port):
  _, labels = _pin(case, port)
  keys = np.sort(labels)
  n = case.n
  if case.u == n:
    assert np.all(keys[1:] != keys[:-1])      # every block of 2048 keys starts with a head
  else:
    # three labels: whether the first key of a block of 2048 continues the run before it
    same = [bool(keys[b] == keys[b - 1]) for b in range(2048, n, 2048)]
    kind = case.id.rsplit("-", 1)[1]
    if n == 4097:
      assert same == ([True, True] if kind == "low" else [False, False])
      assert kind == "high" or keys[2049] != keys[2048]      # a head in the block's second place
    if n == 6145:
      assert same == ([True, True, True] if kind == "low" else [True, True, False])
    if n == 10241:
      assert same == ([True] * 5 if kind == "low" else [True] * 4 + [False])


def test_sort_all_cases_sit_on_the_blocks():
  ns = sorted({c.n for c in SORT_ALL})
  assert ns == [2047, 2048, 2049, 4095, 4096, 4097, 6143, 6144, 6145, 8191, 8192, 10239, 10240, 10241]
  assert [ltv.padded_sort_size(n) for n in (2048, 2049, 4096, 4097, 8192, 10241)] == [2048, 4096, 4096, 8192, 8192, 16384]


KEYS = ltv.key_width_cases()


@pytest.mark.parametrize("case", KEYS, ids=_ids(KEYS))
def test_key_width_cases(case, port):
  _pin(case, port)


def test_key_width_cases_sit_on_the_widths():
  assert sorted((c.u, c.key_width, c.n > ltv.HASH_ABOVE) for c in KEYS) == [
    (255, 1, False), (255, 1, True), (256, 2, False), (256, 2, True), (65535, 2, True), (65536, 4, True)]


EDGE = ltv.edge_value_cases()


@pytest.mark.parametrize("case", EDGE, ids=_ids(EDGE))
def test_edge_value_cases(case, port):
  _pin(case, port)


def test_edge_value_cases_hold_their_values():
  by = {c.id: c for c in EDGE}
  assert by["only-max-hash"].values.tolist() == [ltv.MAX64] and by["only-max-hash"].n == 8193
  assert set(by["max-and-max-1-hash"].values.tolist()) == {ltv.MAX64, ltv.MAX64 - 1} and by["max-and-max-1-hash"].n > ltv.HASH_ABOVE
  assert set(by["zero-and-max-hash"].values.tolist()) == {0, ltv.MAX64}
  v = by["low32-equal-hash"].values
  assert v.size == 3001 and np.all(v & np.uint64(0xFFFFFFFF) == 5)
  assert 0xFFFFFFFF in by["u32-all-ones-hash"].values.tolist() and by["u32-all-ones-hash"].dtype == np.uint32
  assert by["only-u32-all-ones-hash"].stored_width == 4
  for c in EDGE:
    assert (c.n > ltv.HASH_ABOVE) == c.id.endswith("hash"), c.id


SLICES = ltv.many_slices_cases()


@pytest.mark.parametrize("case", SLICES, ids=_ids(SLICES))
def test_many_slices_cases(case, port):
  _pin(case, port)
  assert case.shape[:2] == (9, 8) and case.shape[2] in (255, 256, 257, 512, 513, 1024, 1025)


def test_section_length_solver():
  assert ltv.section_length(3, 1, 1, 2, 32755) == 32768
  assert ltv.section_length(688122, 8, 11, 4, 720895) == ltv.MIB8
  c = ltv.volume_for_length(32768)
  assert (c.shape, c.n, c.u) == ((32755, 1, 1), 32755, 3)
  c = ltv.volume_for_length(ltv.MIB8)
  assert (c.shape, c.n, c.u) == ((256, 256, 11), 720895, 688122)
  for bad in (268, 65549, 700000, (1 << 20) + 1):
    with pytest.raises(ValueError):
      ltv.volume_for_length(bad)
  for wanted, used in ltv.CRC_LENGTHS:
    assert used == wanted or (used == wanted + 3 and wanted % 4 == 1)      # the next multiple of 4
  # the frames: G doubles up to 256 workgroups of 256 x 128 bytes, then the piece grows in steps of 16
  frames = {used: ltv.crc_frame(used) for _, used in ltv.CRC_LENGTHS}
  assert frames == {32768: (1, 128), 32769: (2, 128), 65536: (2, 128), 65537: (4, 128), 1 << 20: (32, 128), (1 << 20) + 4: (64, 128),
                    ltv.MIB8: (256, 128), ltv.MIB8 + 4: (256, 144)}
  ps = [ltv.crc_frame(l)[1] for l in ltv.CRC_ORDER]
  assert sum(a != b for a, b in zip(ps, ps[1:])) >= 2 and set(ltv.CRC_ORDER) == set(frames)


CRC = ltv.crc_cases()


@pytest.mark.parametrize("length", sorted(CRC), ids=[f"L{l}" for l in sorted(CRC)])
def test_crc_cases(length, port):
  case = CRC[length]
  assert case.length == length
  _pin(case, port)


MERGED = ltv.merged_cases()


@pytest.mark.parametrize("case", MERGED, ids=_ids(MERGED))
def test_merged_cases(case, port):
  a, _ = _pin(case.first, port)
  b, _ = _pin(case.second, port)
  whole = case.whole()
  sz = case.first.shape[2]
  assert np.array_equal(whole[:, :, :sz], case.first.volume()) and np.array_equal(whole[:, :, sz:], case.second.volume())
  merged = np.union1d(case.first.values, case.second.values)
  both = np.intersect1d(case.first.values, case.second.values)
  assert 0 < both.size < min(case.first.u, case.second.u)      # the slabs share some labels, not all
  stream = port.compress(whole)
  got = ltv.read_claims(stream)
  assert got["N"] == case.first.n + case.second.n and got["U"] == merged.size
  assert np.array_equal(crackle_amd.labels(stream).astype(np.uint64), merged)
  ns = (case.first.n, case.second.n)
  if case.id == "sorted":
    assert max(ns) <= ltv.HASH_ABOVE
  elif case.id == "unsorted":
    assert min(ns) > ltv.HASH_ABOVE
  else:
    assert case.first.n == 10 and merged.size > 1000 * 4      # a list far longer than the slab has components
