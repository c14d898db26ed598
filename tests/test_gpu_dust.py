"""GPU tests of crackle_amd.dust (ckl_dust: the decoder up to the run tables, k_run_links, k_cc_voxels, k_dust_mark
and k_dust_keys of ckl_components3d.hpp, then the host's stream writer) against the scipy restatement of
tests/dust_numpy.py, which works from the input arrays.  tests/test_dust_cpu.py covers the stream writer on its own
and pins what the shared volumes (tests/dust_volumes.py) are.

Every case asserts: the result decodes (here and with the oracle) to the restated volume in the input's dtype and
memory order, passes ok(), lists exactly the labels that are left, reports the number of removed components, and
recompress(result) is compress(expected) of the oracle byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import crackle_amd
import dust_numpy
import dust_volumes
from crackle_amd import _lib, codec, synth
from crackle_amd import dust      # (the feature under test: without it nothing here runs)
from recompress_volumes import as_signed, floordiv_stream

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CONNECTIVITIES = (6, 18, 26)
ENCODINGS = (dict(), dict(allow_pins=True), dict(markov_model_order=5))


def _run(binary, vol, threshold, connectivity, checker, binary_image=False, invert=False, expect=None):
  """dust() of `binary` (a stream of `vol`) against the restatement; returns (result, number removed)."""
  expected, n_removed = expect if expect is not None else dust_numpy.dust(vol, threshold, connectivity, binary_image, invert)
  out, removed = dust(binary, threshold, connectivity=connectivity, binary_image=binary_image, invert=invert, return_removed=True)
  hi, ho = crackle_amd.header(binary), crackle_amd.header(out)
  assert ho.fortran_order == hi.fortran_order and ho.data_width == hi.data_width
  got = crackle_amd.decompress(out)
  assert got.dtype == vol.dtype and np.array_equal(got, expected)
  assert np.array_equal(checker.decompress(out).reshape(vol.shape, order="F" if ho.fortran_order else "C"), expected)
  assert crackle_amd.ok(out)
  assert np.array_equal(crackle_amd.labels(out), np.unique(expected))
  assert removed == n_removed
  assert crackle_amd.recompress(out) == checker.compress(expected, markov_model_order=hi.markov_model_order)
  return out, removed


@pytest.mark.parametrize("shape,order", [((128, 64, 9), "F"), ((97, 61, 7), "F"), ((96, 80, 6), "C")])
def test_voronoi_with_recurring_labels(checker, shape, order):
  vol = dust_volumes.voronoi(shape, order)
  streams = [checker.compress(vol, **kw) for kw in ENCODINGS]
  assert crackle_amd.header(streams[1]).label_format != crackle_amd.LabelFormat.FLAT
  for conn in CONNECTIVITIES:
    for t, invert in ((50, False), (200, False), (200, True)):
      expect = dust_numpy.dust(vol, t, conn, invert=invert)
      assert expect[1] > 0 and expect[0].any()
      for b in streams:
        _run(b, vol, t, conn, checker, invert=invert, expect=expect)


def test_noise_where_diagonals_decide(checker):
  vol = dust_volumes.noise((64, 48, 5), 3)
  b = checker.compress(vol)
  for conn in CONNECTIVITIES:
    for t in (2, 4):
      for binary_image in (False, True):
        _run(b, vol, t, conn, checker, binary_image=binary_image)
  assert _run(b, vol, 2, 6, checker)[1] == 1175
  assert _run(b, vol, 2, 6, checker, binary_image=True)[1] == 40


def test_noise_with_several_workgroups_a_slice(checker):
  vol = dust_volumes.noise((130, 70, 4), 2)
  b = checker.compress(vol)
  _run(b, vol, 3, 6, checker)
  # at connectivity 26 the foreground is one component of 18 191 voxels, counted across every workgroup and slice
  out, removed = _run(b, vol, 18191, 26, checker)
  assert removed == 0 and out == b
  out, removed = _run(b, vol, 18192, 26, checker)
  assert removed == 1 and not crackle_amd.decompress(out).any()


def test_lds_table_past_its_capacity(checker):
  """Checkerboard (130, 70, 2) of labels 1 and 2: a slice has 9100 runs, a workgroup takes 2048 of them.  At
  connectivity 6 every voxel is a root of its own: 2048 distinct roots for the 1024 entries of k_cc_voxels' LDS
  table, so half of them go to the global counters directly.  At 26 there are two components of 9100 voxels
  each: every run of the volume adds to one of two counters."""
  vol = dust_volumes.checkerboard()
  b = checker.compress(vol)
  out, removed = _run(b, vol, 1, 6, checker)
  assert removed == 0 and out == b
  out, removed = _run(b, vol, 2, 6, checker)
  assert removed == vol.size and crackle_amd.labels(out).tolist() == [0]
  for conn in (18, 26):
    out, removed = _run(b, vol, vol.size // 2, conn, checker)
    assert removed == 0 and out == b
    out, removed = _run(b, vol, vol.size // 2 + 1, conn, checker)
    assert removed == 2
    out, removed = _run(b, vol, vol.size // 2, conn, checker, invert=True)
    assert removed == 2
    out, removed = _run(b, vol, vol.size // 2 + 1, conn, checker, invert=True)
    assert removed == 0 and out == b


def test_threshold_comparison_on_staircase_and_combs(checker):
  stairs = dust_volumes.staircase()
  b = checker.compress(stairs)
  for conn in CONNECTIVITIES:
    assert _run(b, stairs, 79, conn, checker)[1] == 0
    assert _run(b, stairs, 80, conn, checker)[1] == 1
    assert _run(b, stairs, 79, conn, checker, invert=True)[1] == 1
    assert _run(b, stairs, 80, conn, checker, invert=True)[1] == 0
  combs = dust_volumes.combs()
  size = int(np.count_nonzero(combs == 5))
  for kw in ENCODINGS[:2]:
    b = checker.compress(combs, **kw)
    for conn in CONNECTIVITIES:
      assert _run(b, combs, size, conn, checker)[1] == 8               # the specks of label 8 alone
      assert _run(b, combs, size + 1, conn, checker)[1] == 9
      assert _run(b, combs, size, conn, checker, invert=True)[1] == 1
      assert _run(b, combs, size + 1, conn, checker, invert=True)[1] == 0


def test_nothing_removed_gives_the_input_bytes(checker):
  vol = dust_volumes.voronoi((97, 61, 7))
  for kw in (dict(), dict(markov_model_order=5)):
    b = checker.compress(vol, **kw)
    for t in (0, 1):
      for conn in CONNECTIVITIES:
        assert dust(b, t, connectivity=conn) == b
        assert dust(b, t, connectivity=conn, binary_image=True, return_removed=True) == (b, 0)
  # a pin stream comes back FLAT: the same volume, the stream compress() without pins gives
  pins = checker.compress(vol, allow_pins=True)
  assert dust(pins, 1) == checker.compress(vol)


def test_everything_removed(checker):
  vol = dust_volumes.voronoi((97, 61, 7))
  zeros = np.zeros_like(vol)
  for kw in ENCODINGS:
    b = checker.compress(vol, **kw)
    for t, invert in ((2**64 - 1, False), (0, True), (1, True)):
      out, removed = _run(b, vol, t, 26, checker, invert=invert)
      assert removed == dust_numpy.sizes(vol, 26).size and crackle_amd.labels(out).tolist() == [0]
      assert crackle_amd.recompress(out) == checker.compress(zeros, markov_model_order=kw.get("markov_model_order", 0))


def test_pieces_that_touch_at_a_corner_only(checker):
  vol = dust_volumes.corner_pieces()
  removed = {}
  for conn in CONNECTIVITIES:
    for kw in ENCODINGS:
      removed[conn] = _run(checker.compress(vol, **kw), vol, 5, conn, checker)[1]
      _run(checker.compress(vol, **kw), vol, 3, conn, checker)
  assert removed == {6: 5, 18: 2, 26: 1}


def test_small_piece_on_a_big_one(checker):
  vol = dust_volumes.small_on_big()
  for kw in ENCODINGS[:2]:
    b = checker.compress(vol, **kw)
    for conn in CONNECTIVITIES:
      out, removed = _run(b, vol, 4, conn, checker)
      assert removed == 2 and crackle_amd.labels(out).tolist() == [0, 4]
      out, removed = _run(b, vol, 4, conn, checker, binary_image=True)
      assert removed == 1 and crackle_amd.labels(out).tolist() == [0, 4, 7]
      assert _run(b, vol, 4, conn, checker, binary_image=True, invert=True)[1] == 1


def test_label_merged_stream(checker):
  """Touching 2D components that share a label after a label-table rewrite are one component, even at connectivity
  6: equality is by label."""
  lab = synth.as_numpy_f(synth.voronoi_labels((72, 64, 6), np.uint8, seed=8, cell=(8, 8, 2)))
  b = floordiv_stream(checker.compress(lab))
  merged = np.asfortranarray(lab // 2)
  t = int(np.median(dust_numpy.sizes(merged, 26)))
  for conn in CONNECTIVITIES:
    assert _run(b, merged, t, conn, checker)[1] > 0
    _run(b, merged, t, conn, checker, binary_image=True, invert=True)


def test_every_dtype(checker):
  for dt in (np.uint8, np.uint16, np.uint32, np.uint64):
    vol = synth.random_labels((31, 29, 5), dt, seed=3, high=4)
    if dt == np.uint64:
      vol = np.asfortranarray(vol * np.uint64(1 << 40))
      assert int(vol.max()) > 1 << 40
    for kw in ENCODINGS[:2]:
      b = checker.compress(vol, **kw)
      for conn in (6, 26):
        assert _run(b, vol, 3, conn, checker)[1] > 0
      _run(b, vol, 3, 18, checker, binary_image=True)


def test_degenerate_shapes(checker):
  for shape in ((1, 37, 6), (41, 1, 6), (33, 27, 1), (1, 1, 9), (1, 1, 1)):
    vol = synth.random_labels(shape, np.uint16, seed=6, high=3)
    for kw in ENCODINGS[:2]:
      b = checker.compress(vol, **kw)
      for conn in CONNECTIVITIES:
        _run(b, vol, 2, conn, checker)
        _run(b, vol, 2, conn, checker, binary_image=True)
  for vol in (np.zeros((20, 18, 4), np.uint32, order="F"), np.full((20, 18, 4), 77, np.uint64, order="F")):
    b = checker.compress(vol)
    for t in (1440, 1441):
      _run(b, vol, t, 26, checker)
  for shape in ((0, 0, 0), (5, 0, 3), (4, 4, 0)):
    b = checker.compress(np.zeros(shape, np.uint16, order="F"), markov_model_order=3)
    assert dust(b, 7, return_removed=True) == (b, 0)


@pytest.mark.parametrize("shape,n_labels,n_specks,n_after", dust_volumes.WIDTH_EDGES)
def test_key_width_edges_on_the_device(checker, shape, n_labels, n_specks, n_after):
  vol = dust_volumes.width_stripes(shape, n_labels, n_specks)
  expected = dust_volumes.width_stripes_dusted(shape, n_labels, n_specks)      # (pinned against the restatement in tests/test_dust_cpu.py)
  b = checker.compress(vol)
  out, removed = _run(b, vol, 2, 6, checker, expect=(expected, n_specks))
  width = lambda n: np.dtype(np.min_scalar_type(n)).itemsize
  assert crackle_amd.labels(out).size == n_after
  assert (width(codec.num_labels(b)), width(codec.num_labels(out))) == (width(n_labels), width(n_after))


def test_stored_width_drop(checker):
  vol = dust_volumes.stored_width_drop()
  out, removed = _run(checker.compress(vol), vol, 2, 26, checker)
  head = crackle_amd.header(out)
  assert removed == 1 and head.stored_data_width == 1 and head.data_width == 2


def test_medium_volume(checker):
  vol = dust_volumes.voronoi((256, 256, 32), seed=5, cell=(32, 32, 8), modulus=50)
  b = checker.compress(vol)
  for conn in (6, 26):
    assert _run(b, vol, 4000, conn, checker)[1] > 0


def test_repeatable(checker):
  """The same stream three times gives identical bytes: nothing depends on the order atomics land."""
  vol = synth.random_labels((130, 70, 6), np.uint8, seed=11, high=2)
  b = checker.compress(vol)
  outs = [dust(b, 5, connectivity=26, return_removed=True) for _ in range(3)]
  assert outs[0] == outs[1] == outs[2]
  outs = [dust(b, 3, connectivity=6, binary_image=True, return_removed=True) for _ in range(3)]
  assert outs[0] == outs[1] == outs[2]


def test_array_method(checker):
  vol = dust_volumes.voronoi((97, 61, 7))
  arr = crackle_amd.CrackleArray(checker.compress(vol))
  expected, _ = dust_numpy.dust(vol, 200, 18, invert=True)
  got = arr.dust(200, connectivity=18, invert=True)
  assert isinstance(got, crackle_amd.CrackleArray) and got.binary == dust(arr.binary, 200, connectivity=18, invert=True)
  assert got.recompress().binary == checker.compress(expected)


def test_abi_without_a_removed_count(checker):
  vol = dust_volumes.voronoi((97, 61, 7))
  b = checker.compress(vol)
  L = _lib.lib()
  out, n, removed = C.c_void_p(), C.c_uint64(), C.c_uint64()
  flags = _lib.CKL_DUST_INVERT
  assert L.ckl_dust(b, len(b), 200, 26, flags, 0, C.byref(out), C.byref(n), None) == _lib.CKL_OK
  try:
    got = C.string_at(out.value, n.value)
  finally:
    L.ckl_free(out)
  assert L.ckl_dust(b, len(b), 200, 26, flags, 0, C.byref(out), C.byref(n), C.byref(removed)) == _lib.CKL_OK
  try:
    assert got == C.string_at(out.value, n.value)
  finally:
    L.ckl_free(out)
  assert removed.value == 79
  assert (got, 79) == dust(b, 200, invert=True, return_removed=True)


def test_errors(checker):
  lab = synth.as_numpy_f(synth.voronoi_labels((48, 40, 5), np.uint16, seed=12, cell=(8, 8, 2)))
  b = checker.compress(lab)
  # a corrupted label section: slice 1 claims one component more, slice 2 one fewer
  head = crackle_amd.header(b)
  n, off = codec._label_section(b, head)
  at = off + n * head.stored_data_width
  cw = 2      # components per slice are stored at the byte width of sx * sy = 1920
  bad = bytearray(b)
  for z, d in ((1, 1), (2, -1)):
    v = int.from_bytes(bad[at + z * cw:at + (z + 1) * cw], "little") + d
    bad[at + z * cw:at + (z + 1) * cw] = v.to_bytes(cw, "little")
  with pytest.raises(RuntimeError, match="component count does not match the label section"):
    crackle_amd.decompress(bytes(bad))
  with pytest.raises(RuntimeError, match="component count does not match the label section"):
    dust(bytes(bad), 10)
  with pytest.raises(TypeError, match="Signed integer data types are not currently supported"):
    dust(as_signed(b), 10)
  with pytest.raises(ValueError, match="connectivity must be 6, 18 or 26"):
    dust(b, 10, connectivity=8)
