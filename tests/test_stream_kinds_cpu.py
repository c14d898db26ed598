"""What the kinds of tests/stream_kinds.py are: every host kind decodes, by the checker, to the volume it says it
does, has the header flags and the label list its name promises, and the base volumes have what the GPU matrix
(tests/test_gpu_stream_kinds.py) relies on: holes that fill, components that go as dust, voxels that survive an
erosion, false boundaries after // 2, and more than 2048 runs a slice in the large volume.  The host-only readers
labels(), num_labels() and contains() are checked here on every host kind, the lists out of order included."""
import functools

import numpy as np
import pytest

import crackle_amd
import dust_numpy
import erode_numpy
import fill_holes_numpy
import stream_kinds as sk
from crackle_amd import LabelFormat
from oracle import oracle


@functools.lru_cache(maxsize=None)
def _kinds():
  chk = oracle.best()
  return {k.name: k for k in sk.kinds_host(sk.volume_a(), chk) + sk.kinds_large(chk, device=False)}


ALL = sk.HOST_KINDS + sk.LARGE_KINDS[:2]


@pytest.mark.parametrize("name", ALL)
def test_the_checkers_decode_the_kind_to_its_expected_volume(name):
  k = _kinds()[name]
  checkers = [oracle.port()] + ([oracle.ref()] if oracle.ref() is not None else [])
  for chk in checkers:
    got = sk.decode(chk, k.stream)
    assert got.dtype == k.expected.dtype and got.shape == k.expected.shape, chk.kind
    assert np.array_equal(got, k.expected), chk.kind
    assert np.array_equal(sk.decode(chk, k.source), k.base), chk.kind
  assert k.other.shape == k.expected.shape and not np.array_equal(k.other, k.expected)


@pytest.mark.parametrize("name", ALL)
def test_the_header_says_what_the_kind_is(name):
  k = _kinds()[name]
  head = crackle_amd.header(k.stream)
  assert head.is_sorted == (name not in sk.UNSORTED)
  assert (head.label_format != LabelFormat.FLAT) == (name == "pins")
  assert head.format_version == (0 if name == "v0" else 1)
  assert head.markov_model_order == (5 if name == "markov5" else 0)
  assert head.fortran_order == (name != "c-order")
  assert not head.signed


def test_the_label_lists_are_what_the_names_promise():
  kinds = _kinds()
  lists = {name: sk.stored_list(k.stream).astype(np.int64) for name, k in kinds.items()}
  assert (np.diff(lists["flat"]) > 0).all() and (np.diff(lists["remapped"]) > 0).all() and (np.diff(lists["restacked"]) > 0).all()
  assert (np.diff(lists["permuted"]) < 0).any() and len(set(lists["permuted"].tolist())) == len(lists["permuted"])
  assert (np.diff(lists["permuted-merged"]) < 0).any() and len(set(lists["permuted-merged"].tolist())) < len(lists["permuted-merged"])
  assert (np.diff(lists["floordiv"]) >= 0).all() and (np.diff(lists["floordiv"]) == 0).any()
  assert (np.diff(lists["zsplit-mid"]) < 0).any() and 1 < len(lists["zsplit-mid"]) < len(lists["permuted"])
  assert crackle_amd.header(kinds["zsplit-mid"].stream).sz == 1
  assert crackle_amd.header(kinds["zsplit-tail"].stream).sz == 4
  for name, k in kinds.items():
    assert sorted(set(lists[name].tolist()) - ({int(v) for v in np.unique(k.expected)})) == [] or name == "pins", name


@pytest.mark.parametrize("name", ALL)
def test_labels_num_labels_and_contains_on_every_host_kind(name):
  """labels() is the stored list in stored order for FLAT streams, as the reference returns it (crackle/codec.py:17-35);
  contains() finds every label of it whatever the order (crackle/codec.py:98-103)."""
  k = _kinds()[name]
  got = crackle_amd.labels(k.stream)
  assert got.dtype == k.expected.dtype
  if name == "pins":
    assert np.array_equal(got, np.unique(k.expected))
  else:
    assert np.array_equal(got, sk.stored_list(k.stream))
  assert crackle_amd.num_labels(k.stream) == len(got)
  held = set(got.tolist())
  assert held == {int(v) for v in np.unique(k.expected)}
  arr = crackle_amd.CrackleArray(k.stream)
  for v in range(int(got.max()) + 2):
    assert crackle_amd.contains(k.stream, v) == (v in held), v
    assert (v in arr) == (v in held), v
  assert not crackle_amd.contains(k.stream, -1) and not crackle_amd.contains(k.stream, 1 << 40)


@pytest.mark.parametrize("name", ALL)
def test_a_label_the_stream_does_not_hold_is_answered_on_the_host(name):
  """decompress, decompress_range and cutout with label= a value outside the list: an all-False image of the right
  shape at every data width, without a device (the reference's zeros have the stream's data width, and its
  view(bool) raises for every width but 1)."""
  k = _kinds()[name]
  absent = int(k.expected.max()) + 1
  sx, sy, sz = k.expected.shape
  got = crackle_amd.decompress(k.stream, label=absent)
  assert got.dtype == bool and got.shape == (sx, sy, sz) and not got.any()
  assert got.flags.f_contiguous == k.expected.flags.f_contiguous or sz == 1
  part = crackle_amd.decompress_range(k.stream, 0, 1, label=absent)
  assert part.dtype == bool and part.shape == (sx, sy, 1) and not part.any()
  box = sk.box_of(k.expected.shape)
  cut = crackle_amd.cutout(k.stream, box, label=absent)
  assert cut.dtype == bool and cut.shape == k.expected[box].shape and not cut.any()
  assert crackle_amd.decompress(k.stream, label=absent, crop=True).shape == (0, 0, 0)


def test_an_intact_version_0_stream_is_ok():
  """check() answers for version 0 on the host.  The crack codes of a version 0 stream of markov order 0 end exactly
  at the end of the stream, which the reference's index test (crackle/codec.py:926, >=) calls damaged."""
  b = _kinds()["v0"].stream
  assert crackle_amd.check(b) == {"header": True, "crack_index": True, "labels": None, "z": None}
  assert crackle_amd.ok(b)
  assert crackle_amd.check(b[:-1])["crack_index"] is False and not crackle_amd.ok(b[:-1])
  flat = _kinds()["flat"].stream      # version 1: the crc tail follows the codes, and the stream without it is damaged
  tail = 4 * (crackle_amd.header(flat).sz + 1)
  assert crackle_amd.check(flat[:-tail])["crack_index"] is False


def test_the_base_volumes_have_what_the_matrix_relies_on():
  a = sk.volume_a()
  assert a.dtype == np.uint32 and a.flags.f_contiguous and len(np.unique(a)) == 36 and int(a.min()) == 0 and int(a.max()) == 40
  assert len(dust_numpy.sizes(a, 6)) == 105 and len(dust_numpy.sizes(a, 26)) == 101
  sizes = dust_numpy.sizes(a, 26)
  assert int(sizes[0]) == 1 and int(sizes[-1]) == 1433
  dusted, removed = dust_numpy.dust(a, *sk.DUST)
  assert removed == 37 and len(np.unique(dusted)) == 31
  filled = fill_holes_numpy.fill_holes(a, sk.FILL)
  assert filled.filled == 26 and int((filled.volume != a).sum()) == 136
  eroded = erode_numpy.erode(a, 26)
  assert int((eroded != 0).sum()) == 4483 and len(np.unique(eroded)) == 28      # (0 among them)
  assert int((sk.np_erode(a) != 0).sum()) > 0 and not np.array_equal(sk.np_erode(a), a)
  assert len(np.unique(a // 2)) == 20 and sk.false_boundaries(a) == (126, 30)      # 126 along x, 30 more along y
  a8 = sk.volume_a8()
  assert a8.dtype == np.uint8 and np.array_equal(a8, a)
  b = sk.volume_b()
  assert b.flags.c_contiguous and not b.flags.f_contiguous and b.shape == (96, 80, 6)
  assert fill_holes_numpy.fill_holes(b, sk.FILL).filled > 0 and dust_numpy.dust(b, *sk.DUST)[1] > 0
  # the dusted-filled kind fills something dust alone left open or made
  assert fill_holes_numpy.fill_holes(dusted, sk.FILL).filled > 0
  box = sk.box_of(a.shape)
  assert not np.array_equal(sk.other_of(a)[box], (a // 2)[box])


def test_the_large_volume_takes_several_workgroups_of_the_run_kernels():
  big = sk.volume_large()
  assert min(sk.runs_per_slice(big)) > 2048 and min(sk.runs_per_slice(big // 2)) > 2048
  dusted, removed = dust_numpy.dust(big, *sk.DUST)
  assert removed > 0 and len(np.unique(dusted)) > 1 and min(sk.runs_per_slice(dusted)) > 2048
  assert len(np.unique(big // 2)) == 2 and min(sk.false_boundaries(big)) > 0
