"""erode without a GPU: the restatement (tests/erode_numpy.py) pinned on the hand-written volumes of
tests/erode_volumes.py by literal expected arrays and cross-checked against scipy's rank filters, what the generated
volumes of the GPU tests hold (none of them is vacuous), the public surface, the errors decided on the host (through
Python and through the C entry) and the pass-through of empty volumes."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import crackle_amd
import erode_numpy
import erode_volumes as volumes
from crackle_amd import _lib, operations
from crackle_amd.operations import erode      # (the feature under test: without it nothing here runs)
from recompress_volumes import as_signed
from util import golden

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CONNECTIVITIES = volumes.CONNECTIVITIES
BORDERS = (True, False)


def _restate(vol, conn, border):
  out = erode_numpy.erode(vol, conn, border)
  assert out.dtype == vol.dtype and out.shape == vol.shape
  assert out.flags.f_contiguous == vol.flags.f_contiguous and out.flags.c_contiguous == vol.flags.c_contiguous
  return out


# ---- the restatement ----------------------------------------------------------------------------------------------
def test_offsets_of_the_three_elements():
  assert [len(erode_numpy.offsets(c)) for c in CONNECTIVITIES] == [6, 18, 26]
  assert sorted(erode_numpy.offsets(6)) == [(-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (0, 1, 0), (1, 0, 0)]
  assert set(erode_numpy.offsets(26)) == set(volumes.NEIGHBOURS) and len(volumes.NEIGHBOURS) == 26
  assert set(erode_numpy.offsets(26)) - set(erode_numpy.offsets(18)) == {(a, b, c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)}


ONE_SLICE = [      # rows are y, columns x
  [1, 1, 1, 2, 2],
  [1, 1, 1, 2, 2],
  [1, 1, 1, 2, 2],
  [1, 1, 3, 2, 2],
  [1, 1, 1, 2, 2],
]
ONE_SLICE_6 = [
  [1, 1, 0, 0, 2],
  [1, 1, 0, 0, 2],
  [1, 1, 0, 0, 2],
  [1, 0, 0, 0, 2],
  [1, 1, 0, 0, 2],
]
ONE_SLICE_18_26 = [
  [1, 1, 0, 0, 2],
  [1, 1, 0, 0, 2],
  [1, 0, 0, 0, 2],
  [1, 0, 0, 0, 2],
  [1, 0, 0, 0, 2],
]


def _slice(rows):
  return np.asfortranarray(np.array(rows, np.uint8).T[:, :, None])


def test_restatement_one_slice_by_literal_arrays():
  vol = _slice(ONE_SLICE)
  assert vol.shape == (5, 5, 1) and vol[2, 3, 0] == 3
  assert np.array_equal(_restate(vol, 6, False), _slice(ONE_SLICE_6))
  for conn in (18, 26):      # in one slice both are the eight neighbours in the plane
    assert np.array_equal(_restate(vol, conn, False), _slice(ONE_SLICE_18_26))
  for conn in CONNECTIVITIES:      # every voxel of one slice lies on a face
    assert not _restate(vol, conn, True).any()


def test_restatement_single_label():
  vol = volumes.single_label()
  inner = np.zeros(vol.shape, vol.dtype, order="F")
  inner[1:-1, 1:-1, 1:-1] = 7
  assert int(np.count_nonzero(inner)) == 35 * 4 * 3
  for conn in CONNECTIVITIES:
    assert np.array_equal(_restate(vol, conn, True), inner)
    assert np.array_equal(_restate(vol, conn, False), vol)
  for shape in ((37, 6, 1), (37, 1, 5), (1, 6, 5), (1, 1, 1)):
    thin = volumes.single_label(shape)
    for conn in CONNECTIVITIES:
      assert np.array_equal(_restate(thin, conn, False), thin) and not _restate(thin, conn, True).any()


@pytest.mark.parametrize("offset", volumes.NEIGHBOURS, ids=lambda o: "%+d%+d%+d" % o)
def test_restatement_which_neighbour_counts(offset):
  vol = volumes.probe(offset)
  assert vol.shape == (9, 9, 9) and int(np.count_nonzero(vol == 1)) == 124 and int(np.count_nonzero(vol == 3)) == 1
  literal = {      # face, edge-diagonal, corner-diagonal: does the centre survive at 6 / 18 / 26
    1: (False, False, False), 2: (True, False, False), 3: (True, True, False),
  }[sum(map(abs, offset))]
  for conn, survives in zip(CONNECTIVITIES, literal):
    assert volumes.probe_centre_survives(offset, conn) == survives
    for border in BORDERS:
      out = _restate(vol, conn, border)
      assert (out[volumes.PROBE_CENTRE] == 1) == survives
      assert out[tuple(c + o for c, o in zip(volumes.PROBE_CENTRE, offset))] == 0      # the foreign voxel itself always goes


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_restatement_slabs(axis):
  for conn in CONNECTIVITIES:
    for border in BORDERS:
      for thickness in (1, 2):
        assert not (_restate(volumes.slab(axis, thickness), conn, border) == 4).any()
      out = _restate(volumes.slab(axis, 3), conn, border)
      want = np.zeros(volumes.SLAB_SHAPE, bool)
      at = [slice(None) if not border else slice(1, -1)] * 3
      at[axis] = slice(4, 5)      # the middle layer
      want[tuple(at)] = True
      assert np.array_equal(out == 4, want)


def test_restatement_of_the_vanishing_volumes():
  for conn in CONNECTIVITIES:
    for border in BORDERS:
      assert not _restate(volumes.thin_sheets(), conn, border).any()
      wide = volumes.wide_label_on_a_sheet()
      out = _restate(wide, conn, border)
      assert int(wide.max()) == 1 << 40 and np.unique(out).tolist() == [0, 3, 4]
      high = volumes.high_bits_only()
      out = _restate(high, conn, border)
      assert not out[:, 4:6, :].any() and np.unique(out).tolist() == [0, (1 << 32) + 5, (2 << 32) + 5]


def _scipy(vol, conn, border):
  footprint = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[conn])
  kw = dict(mode="constant", cval=0) if border else dict(mode="nearest")
  low, high = ndimage.minimum_filter(vol, footprint=footprint, **kw), ndimage.maximum_filter(vol, footprint=footprint, **kw)
  return np.where((low == high) & (low == vol), vol, 0).astype(vol.dtype)


def _generated():
  for shape, order in volumes.GENERATED:
    yield "voronoi-%dx%dx%d-%s" % (shape + (order,)), volumes.voronoi(shape, order)
  for dt in (np.uint8, np.uint16, np.uint32, np.uint64):
    yield "for_dtype-" + np.dtype(dt).name, volumes.for_dtype(dt)
  yield "strip_path", volumes.strip_path()


def test_restatement_agrees_with_scipy_rank_filters():
  vols = [v for _, v in _generated()] + [volumes.high_bits_only(), volumes.wide_label_on_a_sheet(), volumes.probe((1, 1, 1)), _slice(ONE_SLICE)]
  vols += [volumes.edges((65, 3, 4), v) for v in volumes.EDGE_VARIANTS]
  assert int(volumes.for_dtype(np.uint64).max()) > 1 << 40
  for vol in vols:
    for conn in CONNECTIVITIES:
      for border in BORDERS:
        assert np.array_equal(_restate(vol, conn, border), _scipy(vol, conn, border))


# ---- what the GPU tests rely on ---------------------------------------------------------------------------------------
def test_generated_volumes_are_not_vacuous():
  seen = 0
  for name, vol in _generated():
    for conn in CONNECTIVITIES:
      for border in BORDERS:
        fraction, labels = volumes.survival(vol, _restate(vol, conn, border))
        assert 0.05 <= fraction <= 0.95 and labels >= 2, (name, conn, border, fraction, labels)
        seen += 1
  assert seen == 7 * 6
  runs = volumes.run_pipeline()      # three rows, two slices: every voxel is on a face
  for conn in CONNECTIVITIES:
    fraction, labels = volumes.survival(runs, _restate(runs, conn, False))
    assert 0.05 <= fraction <= 0.95 and labels >= 2
    assert not _restate(runs, conn, True).any()
  assert (volumes.voronoi((70, 50, 13)) == 0).any()      # background among the labels
  # merged labels touch: eroding the merged volume is not eroding first and merging then
  vol = volumes.merging()
  late = volumes.merged(_restate(vol, 26, True))
  assert int(np.count_nonzero(_restate(volumes.merged(vol), 26, True) != late)) > 100


def test_edge_volumes_are_what_they_say():
  for sx in volumes.EDGE_SX:
    vol = volumes.edges((sx, 3, 2), "columns")
    if sx > 32:
      assert vol[31, 0, 0] == 5 and vol[32, 0, 0] == 6
    if sx > 64:
      assert vol[63, 0, 0] == 6 and vol[64, 0, 0] == 5
    assert (vol[sx - 1, 0, 0] == vol[0, 1, 0]) == (sx <= 32 or sx == 65)
    tail = volumes.edges((sx, 3, 2), "row-tail")
    assert tail[sx - 1, 2, 0] == 9 and tail[0, 0, 1] != 9 and tail[sx - 1, 1, 0] != 9
    slices = volumes.edges((sx, 3, 2), "slices")
    assert slices[sx - 1, 2, 0] != slices[0, 0, 1] and not (slices[:, :, 0] == slices[:, :, 1]).any()
  # kept on both sides of a row's end, with one label and with two: the wrap-around pairs of both kinds
  for sx, same in ((31, True), (64, False)):
    vol = volumes.edges((sx, 4, 1), "columns")
    out = _restate(vol, 6, False)
    assert out[sx - 1, 1, 0] and out[0, 2, 0] and (out[sx - 1, 1, 0] == out[0, 2, 0]) == same


def test_format_cases_reach_both_crack_formats():
  from recompress_volumes import interior_x_pairs, linear_pairs, permissible
  seen = {}
  for kind, shape in volumes.FORMAT_CASES:
    for conn in CONNECTIVITIES:
      out = _restate(volumes.format_case(kind, shape), conn, False)
      seen[(kind, shape, conn)] = permissible(out)
      if shape[0] == 1:
        assert interior_x_pairs(out) == 0 and linear_pairs(out) > 0 and out.any()
  assert set(seen.values()) == {True, False}
  assert all(seen[("stripes", (1, 36, 4), conn)] for conn in CONNECTIVITIES)
  # counted without the wrap-arounds, this one would come out on the other side
  out = _restate(volumes.format_case("single", (1, 6, 5)), 6, False)
  assert not permissible(out) and interior_x_pairs(out) == 0 and linear_pairs(out) == 29 >= out.size // 2


# ---- the surface ----------------------------------------------------------------------------------------------------
def test_surface():
  assert crackle_amd.erode is operations.erode and "erode" in crackle_amd.__all__
  sig = inspect.signature(crackle_amd.erode)
  assert list(sig.parameters) == ["binary", "connectivity", "erode_border", "markov_model_order", "device"]
  assert [p.default for p in sig.parameters.values()][1:] == [26, True, None, 0]
  sig = inspect.signature(crackle_amd.CrackleArray.erode)
  assert list(sig.parameters) == ["self", "connectivity", "erode_border"]
  assert [p.default for p in sig.parameters.values()][1:] == [26, True]
  text = open(os.path.join(ROOT, "include", "crackle_amd.h")).read()
  assert re.search(r"\bint\s+ckl_erode\s*\(\s*const uint8_t\*\s*buf,\s*uint64_t n,\s*int connectivity,\s*int flags,\s*int markov_model_order,\s*"
                   r"int device,\s*uint8_t\*\*\s*out,\s*uint64_t\*\s*out_len\s*\)", text)
  assert re.search(r"#define\s+CKL_ERODE_KEEP_BORDER\s+1\b", text) and _lib.CKL_ERODE_KEEP_BORDER == 1
  assert _lib.EXPORTS["ckl_erode"] == (C.c_int, [
    C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)])
  assert hasattr(C.CDLL(_lib.LIB_PATH), "ckl_erode")
  assert _lib.lib().ckl_abi_version() == 1      # an entry was added, none changed
  doc = operations.erode.__doc__
  for words in ("every neighbour", "Equality is by label", "erode_border", "One iteration per call", "byte for byte"):
    assert words in doc


def test_errors_need_no_device():
  binary = golden()["c0_voronoi_u8"]
  for conn in (4, 8, 0, 27, -6):
    with pytest.raises(ValueError, match="connectivity must be 6, 18 or 26"):
      crackle_amd.erode(binary, connectivity=conn)
    with pytest.raises(ValueError, match="connectivity must be 6, 18 or 26"):
      crackle_amd.CrackleArray(binary).erode(connectivity=conn)
  with pytest.raises(ValueError, match="markov_model_order must not be negative"):
    crackle_amd.erode(binary, markov_model_order=-1)
  signed = as_signed(binary)
  assert crackle_amd.header(signed).signed
  with pytest.raises(TypeError, match="Signed integer data types are not currently supported"):
    crackle_amd.erode(signed)
  with pytest.raises(TypeError):
    crackle_amd.CrackleArray(signed).erode()
  # the ABI refuses the same on its own
  out, n = C.c_void_p(), C.c_uint64()
  L = _lib.lib()
  for buf, conn, flags, order in ((binary, 4, 0, -1), (binary, 0, 0, -1), (binary, 27, 1, -1), (signed, 26, 0, -1), (binary, 26, 2, -1), (binary, 6, 0, 16)):
    assert L.ckl_erode(buf, len(buf), conn, flags, order, 0, C.byref(out), C.byref(n)) == _lib.CKL_ERR_ARG
    assert out.value is None and n.value == 0
  assert b"connectivity must be 6, 18 or 26" in (L.ckl_erode(binary, len(binary), 5, 0, -1, 0, C.byref(out), C.byref(n)), L.ckl_last_error())[1]
  assert L.ckl_erode(binary, len(binary), 6, 0, -1, 0, None, C.byref(n)) == _lib.CKL_ERR_ARG
  assert L.ckl_erode(binary[:10], 10, 6, 0, -1, 0, C.byref(out), C.byref(n)) != _lib.CKL_OK


@pytest.mark.parametrize("shape", [(0, 0, 0), (5, 0, 3), (4, 4, 0)])
def test_empty_volumes_come_back_as_recompress_returns_them(checker, shape):
  arr = np.zeros(shape, np.uint16, order="F")
  b = checker.compress(arr, markov_model_order=3)
  want = crackle_amd.recompress(b)
  assert want == b
  for conn in CONNECTIVITIES:
    for border in BORDERS:
      assert crackle_amd.erode(b, connectivity=conn, erode_border=border) == want
  assert crackle_amd.erode(b, markov_model_order=0) == crackle_amd.recompress(b, markov_model_order=0) == checker.compress(arr)
  assert crackle_amd.CrackleArray(b).erode(18, False).binary == want
  # the C entry answers from the host alone too
  out, n = C.c_void_p(), C.c_uint64()
  L = _lib.lib()
  assert L.ckl_erode(b, len(b), 6, _lib.CKL_ERODE_KEEP_BORDER, -1, 0, C.byref(out), C.byref(n)) == _lib.CKL_OK
  try:
    assert C.string_at(out.value, n.value) == want
  finally:
    L.ckl_free(out)
