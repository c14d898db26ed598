"""dust without a GPU: the restatement (tests/dust_numpy.py) pinned on hand-written volumes, the public surface,
the errors decided on the host, and the host half, ckl_relabel_values, which writes the result stream from any
unsigned version 1 stream and one label per 2D component at the input's data width.

The device half computes those labels; here they come from the restatement applied to the decoded golden volumes
and the oracle's 2D component image.  The output must decode (with the oracle) to the restated volume in the input's
dtype, hold the canonical unique list, a valid header crc8 and label crc32c, keep z-index, markov model, crack codes
and slice crcs byte for byte, and be the input itself where no value changes and the input came from compress()."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cc3d_numpy
import crackle_amd
import dust_numpy
import dust_volumes
import golden_cases
from crackle_amd import _lib, codec, operations
from crackle_amd.operations import dust, relabel_values      # (the feature under test: without it nothing here runs)
from recompress_volumes import as_signed
from util import golden

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SMALL = golden_cases.small_cases()


# ---- the restatement ----------------------------------------------------------------------------------------------
def test_restatement_three_and_four():
  vol = dust_volumes.three_and_four()
  three, four = vol.copy(order="F"), vol.copy(order="F")
  three[4:6, 3:5, 1] = 0      # the volume with the 3-voxel piece alone
  four[0:3, 0, 0] = 0
  for conn in (6, 18, 26):
    assert dust_numpy.sizes(vol, conn).tolist() == [3, 4]
    out, removed = dust_numpy.dust(vol, 4, conn)
    assert removed == 1 and np.array_equal(out, four) and out.dtype == vol.dtype and out.flags.f_contiguous
    out, removed = dust_numpy.dust(vol, 4, conn, invert=True)
    assert removed == 1 and np.array_equal(out, three)
    for t in (0, 1, 3):
      out, removed = dust_numpy.dust(vol, t, conn)
      assert removed == 0 and np.array_equal(out, vol)
    out, removed = dust_numpy.dust(vol, 5, conn)
    assert removed == 2 and not out.any()
    out, removed = dust_numpy.dust(vol, 0, conn, invert=True)
    assert removed == 2 and not out.any()


def test_restatement_combs_joined_in_the_last_slice():
  vol = dust_volumes.combs()
  n5 = int(np.count_nonzero(vol == 5))
  for conn in (6, 18, 26):
    assert dust_numpy.sizes(vol, conn).tolist() == [1] * 8 + [n5]      # one piece of label 5, eight specks of label 8
    out, removed = dust_numpy.dust(vol, n5, conn)
    assert removed == 8 and np.array_equal(out, np.where(vol == 5, vol, 0))
    out, removed = dust_numpy.dust(vol, n5 + 1, conn)
    assert removed == 9 and not out.any()
  cut = vol.copy(order="F")
  cut[:, :, 9] = 0
  assert np.count_nonzero(dust_numpy.sizes(cut, 26) == 45) == 17      # without the spines: 17 teeth of 5 x 9 voxels


def test_restatement_corner_pieces():
  vol = dust_volumes.corner_pieces()
  want = {6: [1, 1, 4, 4, 4], 18: [2, 4, 8], 26: [2, 12]}
  for conn, s in want.items():
    assert dust_numpy.sizes(vol, conn).tolist() == s
  out, removed = dust_numpy.dust(vol, 5, 6)
  assert removed == 5 and not out.any()
  out, removed = dust_numpy.dust(vol, 5, 18)
  assert removed == 2 and int(np.count_nonzero(out)) == 8
  out, removed = dust_numpy.dust(vol, 5, 26)
  assert removed == 1 and int(np.count_nonzero(out)) == 12 and out[0, 5, 2] == 0


def test_restatement_small_piece_on_a_big_one():
  vol = dust_volumes.small_on_big()
  out, removed = dust_numpy.dust(vol, 4, 26)
  assert removed == 2 and np.array_equal(out, np.where(vol == 4, vol, 0))
  out, removed = dust_numpy.dust(vol, 4, 26, binary_image=True)      # the piece is part of a component of 51 voxels now
  keep = vol.copy(order="F")
  keep[8, 6, 2] = 0
  assert removed == 1 and np.array_equal(out, keep) and out[5, 2, 1] == 7
  assert dust_numpy.sizes(vol, 26, binary_image=True).tolist() == [1, 51]


# ---- the surface ----------------------------------------------------------------------------------------------------
def test_surface():
  assert crackle_amd.dust is operations.dust and "dust" in crackle_amd.__all__
  assert callable(crackle_amd.CrackleArray.dust)
  text = open(os.path.join(ROOT, "include", "crackle_amd.h")).read()
  assert re.search(r"#define\s+CKL_DUST_BINARY_IMAGE\s+1\b", text) and re.search(r"#define\s+CKL_DUST_INVERT\s+2\b", text)
  assert (_lib.CKL_DUST_BINARY_IMAGE, _lib.CKL_DUST_INVERT) == (1, 2)
  L = C.CDLL(_lib.LIB_PATH)
  for name in ("ckl_dust", "ckl_relabel_values"):
    assert re.search(r"\b%s\s*\(" % name, text) and name in _lib.EXPORTS and hasattr(L, name)


def _v0():
  with np.load(os.path.join(HERE, "golden", "v0.npz")) as z:
    return z[[k for k in z.files if "." not in k][0]].tobytes()


def test_errors_need_no_device():
  binary = golden()["c0_voronoi_u8"]
  with pytest.raises(ValueError, match="threshold must not be negative"):
    crackle_amd.dust(binary, -1)
  with pytest.raises(ValueError, match=r"threshold must be below 2\^64"):
    crackle_amd.dust(binary, 1 << 64)
  for conn in (4, 8, 0):
    with pytest.raises(ValueError, match="connectivity must be 6, 18 or 26"):
      crackle_amd.dust(binary, 5, connectivity=conn)
  v0 = _v0()
  assert crackle_amd.header(v0).format_version == 0
  with pytest.raises(ValueError, match=r"recompress\(\) first"):
    crackle_amd.dust(v0, 5)
  signed = as_signed(binary)
  assert crackle_amd.header(signed).signed
  with pytest.raises(TypeError, match="Signed integer data types are not currently supported"):
    crackle_amd.dust(signed, 5)
  with pytest.raises(TypeError):
    crackle_amd.CrackleArray(signed).dust(5)
  # the ABI refuses the same on its own
  out, n = C.c_void_p(), C.c_uint64()
  L = _lib.lib()
  for buf, conn, flags in ((binary, 4, 0), (binary, 26, 4), (v0, 26, 0), (signed, 26, 0)):
    assert L.ckl_dust(buf, len(buf), 5, conn, flags, 0, C.byref(out), C.byref(n), None) == _lib.CKL_ERR_ARG
  vals = np.zeros(1, np.uint64)
  for buf in (v0, signed):
    assert L.ckl_relabel_values(buf, len(buf), vals.ctypes.data, 1, C.byref(out), C.byref(n)) == _lib.CKL_ERR_ARG


@pytest.mark.parametrize("shape", [(0, 0, 0), (5, 0, 3), (4, 4, 0)])
def test_empty_volumes_come_back_unchanged(checker, shape):
  b = checker.compress(np.zeros(shape, np.uint16, order="F"), markov_model_order=3)
  assert crackle_amd.dust(b, 10) == b
  assert crackle_amd.dust(b, 10, connectivity=6, binary_image=True, invert=True, return_removed=True) == (b, 0)
  assert crackle_amd.CrackleArray(b).dust(3).binary == b
  assert operations.relabel_values(b, np.zeros(0, np.uint64)) == b


# ---- ckl_relabel_values -------------------------------------------------------------------------------------------------
# name -> (threshold, connectivity, binary_image, invert): FLAT and pins, C order, every data width
CASES = {
  "rand_17x13x5_uint8_F_m0_p0": (2, 26, False, False),
  "rand_17x13x5_uint16_C_m5_p1": (3, 6, False, False),
  "rand_17x13x5_uint32_F_m5_p0": (2, 18, False, False),
  "rand_17x13x5_uint64_F_m0_p1": (2, 6, False, True),
  "rand_64x63x3_m3": (2, 6, False, False),
  "c0_voronoi_u8": (170, 26, False, False),
  "c0_voronoi_u8_m5": (170, 6, False, True),
  "c0_voronoi_u8_pins": (170, 18, False, False),
  "c0_voronoi_u8_c": (170, 26, False, False),
  "dots_30_pins": (2, 18, True, False),
}


def _volume(checker, binary):
  h = crackle_amd.header(binary)
  return checker.decompress(binary).reshape((h.sx, h.sy, h.sz), order="F" if h.fortran_order else "C")


def _component_values(checker, vol, expected):
  """The value every 2D component of vol (stream order) has in `expected`."""
  cc2d, per, _ = checker.connected_components(np.asfortranarray(vol))
  return cc3d_numpy.component_ids(expected, cc2d, per)


def _sections(binary):
  """(z-index with its crc, label section, model + crack codes, label crc, slice crcs)"""
  h = crackle_amd.header(binary)
  a = h.header_bytes
  b = a + h.grid_index_bytes
  c = b + h.num_label_bytes
  d = len(binary) - 4 * (h.sz + 1)
  return binary[a:b], binary[b:c], binary[c:d], int.from_bytes(binary[d:d + 4], "little"), binary[d + 4:]


def _check(checker, binary, out, expected):
  hi, ho = crackle_amd.header(binary), crackle_amd.header(out)      # (header() verifies the crc8)
  uniq = np.unique(expected)
  assert ho.format_version == 1 and ho.label_format == crackle_amd.LabelFormat.FLAT and ho.is_sorted and not ho.signed
  assert ho.data_width == hi.data_width and ho.fortran_order == hi.fortran_order
  assert ho.stored_data_width == np.dtype(np.min_scalar_type(int(uniq[-1]))).itemsize
  assert (ho.sx, ho.sy, ho.sz, ho.crack_format, ho.markov_model_order) == (hi.sx, hi.sy, hi.sz, hi.crack_format, hi.markov_model_order)
  zi, _, cracks_i, _, crcs_i = _sections(binary)
  zo, lab_o, cracks_o, lab_crc, crcs_o = _sections(out)
  assert zo == zi and cracks_o == cracks_i and crcs_o == crcs_i
  assert lab_crc == int(_lib.lib().ckl_crc32c(lab_o, len(lab_o))) == codec.labels_crc(out)
  report = crackle_amd.check(out)
  assert report["header"] is True and report["crack_index"] is True and report["labels"] is True
  got_labels = crackle_amd.labels(out)
  assert got_labels.dtype == expected.dtype and np.array_equal(got_labels, uniq) and np.all(np.diff(got_labels.astype(np.float64)) > 0)
  kw = np.dtype(np.min_scalar_type(uniq.size)).itemsize
  cw = np.dtype(np.min_scalar_type(hi.sx * hi.sy)).itemsize
  n_comp = (len(lab_o) - 8 - uniq.size * ho.stored_data_width - cw * hi.sz) // kw
  assert ho.num_label_bytes == 8 + uniq.size * ho.stored_data_width + cw * hi.sz + n_comp * kw
  got = _volume(checker, out)
  assert got.dtype == expected.dtype and np.array_equal(got, expected)


def test_cases_cover_the_formats():
  heads = [crackle_amd.header(golden()[name]) for name in CASES]
  assert {h.label_format for h in heads} == {crackle_amd.LabelFormat.FLAT, crackle_amd.LabelFormat.PINS_VARIABLE_WIDTH}
  assert {h.fortran_order for h in heads} == {True, False}
  assert {h.data_width for h in heads} == {1, 2, 4, 8}


@pytest.mark.parametrize("name", sorted(CASES))
def test_relabel_values_on_golden_streams(checker, name):
  binary = golden()[name]
  t, conn, binary_image, invert = CASES[name]
  vol = _volume(checker, binary)
  assert np.array_equal(vol, SMALL[name][0])
  expected, removed = dust_numpy.dust(vol, t, conn, binary_image, invert)
  assert removed > 0 and expected.any(), "the case removes something and keeps something"
  out = operations.relabel_values(binary, _component_values(checker, vol, expected))
  _check(checker, binary, out, expected)
  # unchanged values: the canonical form of the input, which is the input where it is a FLAT stream from compress()
  same = operations.relabel_values(binary, _component_values(checker, vol, vol))
  _check(checker, binary, same, vol)
  head = crackle_amd.header(binary)
  if head.label_format == crackle_amd.LabelFormat.FLAT:
    assert same == binary
    assert same == checker.compress(vol, markov_model_order=head.markov_model_order)


def test_relabel_values_refuses_what_does_not_fit(checker):
  binary = golden()["c0_voronoi_u8"]
  vol = _volume(checker, binary)
  vals = _component_values(checker, vol, vol)
  for bad in (vals[:-1], np.append(vals, 1), np.zeros(0, np.uint64)):
    with pytest.raises(ValueError, match=rf"{bad.size} ids for the stream's {vals.size} components"):
      operations.relabel_values(binary, bad)
  over = vals.copy()
  over[3] = 256
  with pytest.raises(ValueError, match="does not fit the stream's data width of 1 bytes"):
    operations.relabel_values(binary, over)
  wide = checker.compress(vol.astype(np.uint64))
  over[3] = 2**64 - 1
  out = operations.relabel_values(wide, over)
  assert crackle_amd.header(out).stored_data_width == 8 and int(crackle_amd.labels(out)[-1]) == 2**64 - 1


# ---- widths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n_labels,n_specks,n_after", dust_volumes.WIDTH_EDGES)
def test_key_width_edges_of_the_section_writer(checker, shape, n_labels, n_specks, n_after):
  vol = dust_volumes.width_stripes(shape, n_labels, n_specks)
  assert np.unique(vol).size == n_labels and vol.all()
  s = dust_numpy.sizes(vol, 6)
  assert s.size == n_labels and s[:n_specks].tolist() == [1] * n_specks and s[n_specks] >= 3      # the specks, then the stripes that lost a voxel
  expected, removed = dust_numpy.dust(vol, 2, 6)
  assert removed == n_specks and np.unique(expected).size == n_after
  assert np.array_equal(expected, dust_volumes.width_stripes_dusted(shape, n_labels, n_specks))      # what the GPU test compares with
  binary = checker.compress(vol)
  out = operations.relabel_values(binary, _component_values(checker, vol, expected))
  _check(checker, binary, out, expected)
  width = lambda n: np.dtype(np.min_scalar_type(n)).itemsize
  n_comp = _component_values(checker, vol, vol).size
  assert len(_sections(binary)[1]) - len(_sections(out)[1]) == (
    (n_labels * crackle_amd.header(binary).stored_data_width + n_comp * width(n_labels))
    - (n_after * crackle_amd.header(out).stored_data_width + n_comp * width(n_after)))


def test_stored_width_drops_with_the_last_wide_label(checker):
  vol = dust_volumes.stored_width_drop()
  expected, removed = dust_numpy.dust(vol, 2, 26)
  assert removed == 1 and np.unique(expected).tolist() == [0, 3, 200]
  binary = checker.compress(vol)
  assert crackle_amd.header(binary).stored_data_width == 2
  out = operations.relabel_values(binary, _component_values(checker, vol, expected))
  _check(checker, binary, out, expected)
  ho = crackle_amd.header(out)
  assert ho.stored_data_width == 1 and ho.data_width == 2


# ---- what the GPU tests rely on ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dust_volumes.GPU_CASES, ids=[c[0] for c in dust_volumes.GPU_CASES])
def test_gpu_volumes_have_removed_and_kept_components(case):
  _, make, t, conn, binary_image = case
  vol = make()
  s = dust_numpy.sizes(vol, conn, binary_image)
  assert 0 < np.count_nonzero(s < t) < s.size


def test_figures_of_the_shared_gpu_volumes():
  vol = dust_volumes.voronoi((97, 61, 7))
  expected, removed = dust_numpy.dust(vol, 200, 26)
  s = dust_numpy.sizes(vol, 26)
  assert (removed, int(np.count_nonzero(s >= 200))) == (115, 79)
  before, after = set(np.unique(vol).tolist()), set(np.unique(expected).tolist())
  # labels 2, 7 and 31 have no piece of 200 voxels (their largest: 188, 148, 36): they leave the list, and 0 enters
  assert before - after == {2, 7, 31} and after - before == {0}
  vol = dust_volumes.noise((64, 48, 5), 3)
  s = dust_numpy.sizes(vol, 6)
  assert (int(np.count_nonzero(s < 2)), int(np.count_nonzero(s >= 2))) == (1175, 774)
  s = dust_numpy.sizes(vol, 6, binary_image=True)
  assert (int(np.count_nonzero(s < 2)), int(np.count_nonzero(s >= 2))) == (40, 4)
  vol = dust_volumes.noise((130, 70, 4), 2)
  assert np.count_nonzero(np.diff(vol[:, :, 0].ravel(order="F").astype(np.int16))) > 2048      # several workgroups a slice
  assert dust_numpy.sizes(vol, 26).tolist() == [18191]
  vol = dust_volumes.checkerboard()
  assert not (vol == 0).any()
  assert dust_numpy.sizes(vol, 6).tolist() == [1] * vol.size and vol[:, :, 0].size > 2048
  assert dust_numpy.sizes(vol, 26).tolist() == [vol.size // 2] * 2
  assert dust_numpy.sizes(dust_volumes.staircase(), 6).tolist() == [79]
