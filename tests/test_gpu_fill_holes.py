"""GPU tests of crackle_amd.fill_holes (ckl_fill_holes: the decoder up to the run tables, k_run_links in its
background mode, k_hole_scan, k_edit_mark and k_edit_keys of ckl_components3d.hpp, then the host's stream writer)
against the scipy restatement of tests/fill_holes_numpy.py, which works from the input arrays.
tests/test_fill_holes_cpu.py pins what the shared volumes (tests/fill_holes_volumes.py) are.

Every case asserts: the result decodes (here and with the oracle) to the restated volume in the input's dtype and
memory order, passes ok(), lists exactly the labels that are left, reports the number of filled holes,
recompress(result) is compress(expected) of the oracle byte for byte, filling again changes nothing, and the output
is the input where nothing is fillable and the input is a FLAT stream from compress()."""
import ctypes as C

import numpy as np
import pytest

import cc3d_numpy
import crackle_amd
import dust_numpy
import dust_volumes
import fill_holes_numpy
import fill_holes_volumes as volumes
from crackle_amd import _lib, codec
from crackle_amd import fill_holes      # (the feature under test: without it nothing here runs)

pytestmark = pytest.mark.gpu

CONNECTIVITIES = (6, 18, 26)
ENCODINGS = (dict(), dict(allow_pins=True), dict(markov_model_order=5))


def _run(binary, vol, connectivity, checker, expect=None):
  """fill_holes() of `binary` (a stream of `vol`) against the restatement; returns (result, holes filled)."""
  expected, n_filled = expect if expect is not None else fill_holes_numpy.fill_holes(vol, connectivity)[:2]
  out, filled = fill_holes(binary, connectivity=connectivity, return_filled=True)
  assert fill_holes(binary, connectivity=connectivity) == out
  hi, ho = crackle_amd.header(binary), crackle_amd.header(out)
  assert ho.fortran_order == hi.fortran_order and ho.data_width == hi.data_width
  assert ho.format_version == 1 and ho.label_format == crackle_amd.LabelFormat.FLAT and ho.is_sorted
  got = crackle_amd.decompress(out)
  assert got.dtype == vol.dtype and got.flags.f_contiguous == vol.flags.f_contiguous and np.array_equal(got, expected)
  assert np.array_equal(checker.decompress(out).reshape(vol.shape, order="F" if ho.fortran_order else "C"), expected)
  assert crackle_amd.ok(out)
  assert np.array_equal(crackle_amd.labels(out), np.unique(expected))
  assert filled == n_filled
  assert crackle_amd.recompress(out) == checker.compress(expected, markov_model_order=hi.markov_model_order)
  assert fill_holes(out, connectivity=connectivity, return_filled=True) == (out, 0)
  if n_filled == 0 and hi.label_format == crackle_amd.LabelFormat.FLAT:
    assert out == binary
  return out, filled


def _all(vol, checker, encodings=ENCODINGS, connectivities=CONNECTIVITIES):
  """Every connectivity on every encoding of vol; returns {connectivity: holes filled}."""
  streams = [checker.compress(vol, **kw) for kw in encodings]
  filled = {}
  for conn in connectivities:
    expect = fill_holes_numpy.fill_holes(vol, conn)[:2]
    for b in streams:
      filled[conn] = _run(b, vol, conn, checker, expect=expect)[1]
  return filled


# ---- hand-written minimal cases: one per way the scan can go wrong --------------------------------------------------
def test_one_voxel_hole(checker):
  assert _all(volumes.one_voxel(), checker) == {6: 1, 18: 1, 26: 1}


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("last", [False, True])
def test_hole_at_a_face_stays_and_next_to_it_fills(checker, axis, last):
  assert _all(volumes.at_face(axis, last), checker, ENCODINGS[:2]) == {6: 0, 18: 0, 26: 0}
  assert _all(volumes.at_face(axis, last, inset=1), checker, ENCODINGS[:2]) == {6: 1, 18: 1, 26: 1}


@pytest.mark.parametrize("direction", sorted(volumes.FACE_STEPS))
def test_second_label_through_one_face_keeps_the_hole(checker, direction):
  assert _all(volumes.second_label_by_face(direction), checker) == {6: 0, 18: 0, 26: 0}


def test_second_label_in_diagonal_contact_does_not(checker):
  assert _all(volumes.second_label_diagonal(), checker) == {6: 1, 18: 1, 26: 1}


def test_hole_through_three_slices(checker):
  assert _all(volumes.three_slices(), checker) == {6: 1, 18: 1, 26: 1}


def test_holes_touching_at_an_edge_or_a_corner(checker):
  assert _all(volumes.edge_touching_holes(), checker) == {6: 1, 18: 0, 26: 0}
  assert _all(volumes.corner_touching_holes(), checker) == {6: 1, 18: 1, 26: 0}


def test_one_slice_has_no_fillable_hole(checker):
  vol = np.full((33, 9, 1), 3, np.uint8, order="F")
  vol[4:30, 4, 0] = 0
  assert _all(vol, checker, ENCODINGS[:2]) == {6: 0, 18: 0, 26: 0}


# ---- the output of mask() and dust(): holes cut up by false boundaries ------------------------------------------------------
def test_holes_left_by_mask_and_dust(checker):
  full = volumes.block()
  for make, threshold in ((volumes.speck_in_block, 2), (volumes.bar_in_void, 4)):
    vol = make()
    hole = np.asfortranarray(np.where(vol == 7, 0, vol).astype(vol.dtype))
    for kw in (dict(), dict(markov_model_order=5)):
      b = checker.compress(vol, **kw)
      for edited in (crackle_amd.mask(b, [7]), crackle_amd.dust(b, threshold, connectivity=6)):
        assert np.array_equal(crackle_amd.decompress(edited), hole)
        if make is volumes.bar_in_void:
          assert edited != checker.compress(hole, **kw)      # the bar's cracks are still there (the speck's are the hole's own)
        for conn in CONNECTIVITIES:
          out, filled = _run(edited, hole, conn, checker, expect=(full, 1))
          assert crackle_amd.labels(out).tolist() == [4]
  # before the edit the void of bar_in_void touches labels 4 and 7: it stays
  assert _all(volumes.bar_in_void(), checker, ENCODINGS[:1]) == {6: 0, 18: 0, 26: 0}


# ---- generated volumes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,order", volumes.PUNCHED)
def test_voronoi_with_punched_voids(checker, shape, order):
  vol = volumes.punched(shape, order)
  assert crackle_amd.header(checker.compress(vol, allow_pins=True)).label_format != crackle_amd.LabelFormat.FLAT
  filled = _all(vol, checker)
  assert min(filled.values()) >= 10
  if shape == (128, 64, 9):
    assert filled[6] == 30


def test_several_workgroups_a_slice(checker):
  """More than 2048 runs a slice (kContactRuns): noise, and thousands of filled roots with one enclosing label."""
  assert _all(dust_volumes.noise((130, 70, 4), 2), checker, ENCODINGS[:1]) == {6: 150, 18: 1, 26: 0}
  assert _all(volumes.pocked(), checker, ENCODINGS[:2]) == {6: 4352, 18: 4352, 26: 1}


def test_one_hole_of_many_runs(checker):
  """The cavity of the hollow box is ONE hole whose runs of label 0 (more than 4000 a slice, three slices) are spread
  over nine workgroups, all updating one state word.  This is the case the early-out and the monotone state word of
  k_hole_scan exist for: thousands of threads report "label 6" for the same root at once (only the first changes the
  word, the others read it and send nothing), and in the two variants a single run among them reports a second label
  or a face of the volume, early or late among the others.  The word has to end as MANY or OPEN whatever the order,
  and no run that saw "label 6" first may put it back."""
  for kw in ENCODINGS[:2]:
    b = checker.compress(volumes.hollow_box(), **kw)
    for conn in CONNECTIVITIES:
      out, filled = _run(b, volumes.hollow_box(), conn, checker)
      assert filled == 1 and crackle_amd.labels(out).tolist() == [6]
  for variant in ("second-label", "tunnel"):
    vol = volumes.hollow_box(variant)
    b = checker.compress(vol)
    for conn in CONNECTIVITIES:
      out, filled = _run(b, vol, conn, checker)
      assert filled == 0 and out == b
  # three runs give identical bytes: nothing depends on the order in which the atomics land
  b = checker.compress(volumes.hollow_box("second-label"))
  outs = [fill_holes(b, connectivity=18, return_filled=True) for _ in range(3)]
  assert outs[0] == outs[1] == outs[2]


@pytest.mark.parametrize("n_labels,widths", [(256, (2, 2)), (255, (2, 1))])
def test_label_zero_leaves_the_list(checker, n_labels, widths):
  """Every background voxel is a fillable hole.  The request named 256 labels plus background for a key width that
  drops from 2 bytes to 1; one-byte keys end at 255 values (tests/dust_volumes.py, WIDTH_EDGES), so 256 labels keep
  2-byte keys (257 values, then 256) and the drop is at 255 labels (256 values, then 255).  Both are run."""
  vol = volumes.all_holes_fillable(n_labels)
  width = lambda n: np.dtype(np.min_scalar_type(n)).itemsize
  for kw in ENCODINGS[:2]:
    b = checker.compress(vol, **kw)
    for conn in CONNECTIVITIES:
      out, filled = _run(b, vol, conn, checker)
      assert filled == 256 and crackle_amd.labels(out).tolist() == list(range(1, n_labels + 1))
      assert (codec.num_labels(b), codec.num_labels(out)) == (n_labels + 1, n_labels)
      assert (width(codec.num_labels(b)), width(codec.num_labels(out))) == widths
      # the section's own length says the same: 8 + the list + 2-byte slice counts (sx * sy = 4096) + one key per component
      head = crackle_amd.header(out)
      at = head.header_bytes + head.grid_index_bytes + 8 + n_labels * head.stored_data_width
      n_comp = sum(int.from_bytes(out[at + 2 * z:at + 2 * z + 2], "little") for z in range(3))
      assert n_comp >= 1020 and head.num_label_bytes == 8 + n_labels * head.stored_data_width + 6 + n_comp * widths[1]


def test_nothing_to_fill_gives_the_input_bytes(checker):
  no_zero = dust_volumes.checkerboard()
  assert not (no_zero == 0).any()
  all_zero = np.zeros((20, 18, 4), np.uint32, order="F")
  for vol in (no_zero, all_zero, dust_volumes.voronoi((97, 61, 7))):
    for kw in (dict(), dict(markov_model_order=5)):
      b = checker.compress(vol, **kw)
      for conn in CONNECTIVITIES:
        assert fill_holes(b, connectivity=conn, return_filled=True) == (b, 0)
    _all(vol, checker, ENCODINGS[:1], (6,))
  # a pin stream comes back FLAT: the same volume, the stream compress() without pins gives
  vol = dust_volumes.voronoi((97, 61, 7))
  pins = checker.compress(vol, allow_pins=True)
  assert crackle_amd.header(pins).label_format != crackle_amd.LabelFormat.FLAT
  assert fill_holes(pins) == checker.compress(vol)


def test_every_dtype(checker):
  for dt in (np.uint8, np.uint16, np.uint32, np.uint64):
    vol = volumes.for_dtype(dt)
    assert _all(vol, checker, ENCODINGS[:2]) == {6: 2, 18: 2, 26: 2}
    c_order = np.ascontiguousarray(vol)
    assert _all(c_order, checker, ENCODINGS[:1], (6,)) == {6: 2}


def test_array_method_and_abi_without_a_count(checker):
  vol = volumes.punched((97, 61, 7))
  expected = fill_holes_numpy.fill_holes(vol, 18).volume
  arr = crackle_amd.CrackleArray(checker.compress(vol))
  got = arr.fill_holes(connectivity=18)
  assert isinstance(got, crackle_amd.CrackleArray) and got.binary == fill_holes(arr.binary, connectivity=18)
  assert got.recompress().binary == checker.compress(expected)
  assert arr.fill_holes().binary == fill_holes(arr.binary, connectivity=6)      # the default is the background's 6
  L = _lib.lib()
  out, n = C.c_void_p(), C.c_uint64()
  assert L.ckl_fill_holes(arr.binary, len(arr.binary), 18, 0, C.byref(out), C.byref(n), None) == _lib.CKL_OK
  try:
    assert C.string_at(out.value, n.value) == got.binary
  finally:
    L.ckl_free(out)


# ---- the kernels whose arguments changed ----------------------------------------------------------------------------------------
def test_dust_and_connected_components_are_what_they_were(checker):
  """k_run_links got a mode and link_row a shared row walk; dust's mark and key kernels became the generic ones.  Both
  functions against their own restatements on two of the shared volumes (one with several workgroups a slice)."""
  for vol in (volumes.punched((97, 61, 7)), dust_volumes.noise((130, 70, 4), 2)):
    b = checker.compress(vol)
    for conn in CONNECTIVITIES:
      want, mapping = cc3d_numpy.connected_components(vol, conn)
      out, got_map = crackle_amd.connected_components(b, connectivity=conn, return_mapping=True)
      assert got_map == mapping and np.array_equal(crackle_amd.decompress(out), want)
      assert crackle_amd.ok(out) and crackle_amd.recompress(out) == checker.compress(want)
      for threshold, binary_image, invert in ((3, False, False), (20, True, False), (20, False, True)):
        expected, n_removed = dust_numpy.dust(vol, threshold, conn, binary_image, invert)
        out, removed = crackle_amd.dust(b, threshold, connectivity=conn, binary_image=binary_image, invert=invert, return_removed=True)
        assert removed == n_removed and np.array_equal(crackle_amd.decompress(out), expected)
        assert np.array_equal(crackle_amd.labels(out), np.unique(expected))
        assert crackle_amd.recompress(out) == checker.compress(expected)
