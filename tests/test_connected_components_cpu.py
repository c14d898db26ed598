"""connected_components without a GPU: the host half, ckl_relabel_components, which writes the result
stream from any version 1 stream and one new id per 2D component.

The device half computes those ids; here they come from the scipy restatement (tests/cc3d_numpy.py) of
the decoded golden volumes and the oracle's 2D component image.  The output must decode (with the
oracle) to the restated volume, carry the specified header, keep the input's z-index, markov model,
crack codes and slice crcs byte for byte, hold a valid label crc32c, and equal
compress(expected.astype(uint32), markov_model_order=m) of the oracle wherever that picks the input's
crack format.

The encoder takes the crack format from pixel_pairs < voxels / 2 (src/crackle.hpp:48-55), and
relabelling can lower pixel_pairs at row and slice wrap-arounds.  The cases below sit away from that
threshold (noise with few equal neighbours on one side, Voronoi cells and uniform volumes on the
other), and the tests assert that the formats agree for every one of them before comparing bytes."""
import numpy as np
import pytest

import cc3d_numpy
import crackle_amd
import golden_cases
from crackle_amd import _lib, codec, operations
from util import golden

SMALL = golden_cases.small_cases()

# name -> connectivity: flat and pins, markov orders 0 and 5 (and 3), both crack formats, both orders
CASES = {
  "rand_17x13x5_uint8_F_m0_p0": 26,
  "rand_17x13x5_uint16_C_m5_p1": 26,
  "rand_17x13x5_uint32_F_m5_p0": 18,
  "rand_17x13x5_uint64_F_m0_p1": 6,
  "rand_64x63x3_m3": 26,
  "rand_254x257x2_m0": 6,
  "noise_2000_m5": 26,
  "binary_noise": 18,
  "c0_voronoi_u8": 26,
  "c0_voronoi_u8_m5": 6,
  "c0_voronoi_u8_pins": 18,
  "c0_voronoi_u8_pins_m5": 26,
  "c0_voronoi_u8_c": 26,
  "dots_30_pins": 26,
  "zeros_50": 26,
  "kat_ones_300": 6,
}


def _volume(checker, binary):
  """The oracle's decode of a stream as an (sx, sy, sz) array."""
  h = crackle_amd.header(binary)
  return checker.decompress(binary).reshape((h.sx, h.sy, h.sz), order="F" if h.fortran_order else "C")


def _ids(checker, vol, connectivity):
  """(restated volume, one 3D id per 2D component in stream order)."""
  ccl, _ = cc3d_numpy.connected_components(vol, connectivity)
  cc2d, per, _ = checker.connected_components(np.asfortranarray(vol))
  return ccl, cc3d_numpy.component_ids(ccl, cc2d, per)


def _sections(binary):
  """(z-index with its crc, label section, model + crack codes, label crc, slice crcs)"""
  h = crackle_amd.header(binary)
  a = h.header_bytes
  b = a + h.grid_index_bytes
  c = b + h.num_label_bytes
  d = len(binary) - 4 * (h.sz + 1)
  return binary[a:b], binary[b:c], binary[c:d], int.from_bytes(binary[d:d + 4], "little"), binary[d + 4:]


def _check(checker, binary, out, ccl, n_comp_2d):
  hi, ho = crackle_amd.header(binary), crackle_amd.header(out)
  n = int(ccl.max())
  uniq = np.unique(ccl)
  assert ho.format_version == 1 and ho.data_width == 4 and not ho.signed
  assert ho.stored_data_width == np.dtype(np.min_scalar_type(n)).itemsize
  assert ho.label_format == crackle_amd.LabelFormat.FLAT and ho.is_sorted
  assert (ho.sx, ho.sy, ho.sz) == (hi.sx, hi.sy, hi.sz)
  assert (ho.crack_format, ho.markov_model_order, ho.fortran_order) == (hi.crack_format, hi.markov_model_order, hi.fortran_order)
  cw = np.dtype(np.min_scalar_type(hi.sx * hi.sy)).itemsize
  kw = np.dtype(np.min_scalar_type(uniq.size)).itemsize
  assert ho.num_label_bytes == 8 + uniq.size * ho.stored_data_width + cw * hi.sz + n_comp_2d * kw
  zi, _, cracks_i, _, crcs_i = _sections(binary)
  zo, lab_o, cracks_o, lab_crc, crcs_o = _sections(out)
  assert zo == zi and cracks_o == cracks_i and crcs_o == crcs_i
  assert lab_crc == int(_lib.lib().ckl_crc32c(lab_o, len(lab_o))) == codec.labels_crc(out)
  assert np.array_equal(crackle_amd.labels(out), uniq)
  assert np.array_equal(_volume(checker, out), ccl)


def _reference(checker, ccl, head):
  expected = ccl if head.fortran_order else np.ascontiguousarray(ccl)
  return checker.compress(expected, markov_model_order=head.markov_model_order)


def test_cases_cover_the_formats():
  heads = [crackle_amd.header(golden()[name]) for name in CASES]
  assert {h.label_format for h in heads} == {crackle_amd.LabelFormat.FLAT, crackle_amd.LabelFormat.PINS_VARIABLE_WIDTH}
  assert {h.crack_format for h in heads} == {crackle_amd.CrackFormat.IMPERMISSIBLE, crackle_amd.CrackFormat.PERMISSIBLE}
  assert {0, 5} <= {h.markov_model_order for h in heads}
  assert {h.fortran_order for h in heads} == {True, False}


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_streams(checker, name):
  binary = golden()[name]
  head = crackle_amd.header(binary)
  vol = _volume(checker, binary)
  assert np.array_equal(vol, SMALL[name][0])
  ccl, ids = _ids(checker, vol, CASES[name])
  out = operations.relabel_components(binary, ids)
  _check(checker, binary, out, ccl, ids.size)
  ref = _reference(checker, ccl, head)
  assert crackle_amd.header(ref).crack_format == head.crack_format, "the case sits on the crack format threshold: pick another"
  assert out == ref


def isolated_voxels(shape, n):
  """n single voxels of label 7 on a zero background, none touching another even at a corner."""
  vol = np.zeros(shape, np.uint8, order="F")
  xs, ys = np.meshgrid(np.arange(0, shape[0], 2), np.arange(0, shape[1], 2), indexing="ij")
  xs, ys = xs.ravel(order="F")[:n], ys.ravel(order="F")[:n]
  assert xs.size == n
  vol[xs, ys, 0] = 7
  return vol


def stripes(shape, n):
  """n components without a zero voxel: the rows cut into 1-voxel-wide stripes of sx*sy/m voxels, m the
  next power of two >= n, labels 3 and 5 alternating along and across the rows; the last m - n + 1
  stripes are one piece of label 9.  (6-connectivity: stripes of one label touch at corners.)"""
  m = 1 << (n - 1).bit_length()
  length = shape[0] * shape[1] // m
  seg = np.arange(shape[0] * shape[1]) // length
  per_row = shape[0] // length
  lab = np.where((seg % per_row + seg // per_row) % 2 == 0, 3, 5).astype(np.uint8)
  assert m - n + 1 <= per_row
  lab[seg >= n - 1] = 9
  return np.asfortranarray(lab.reshape(shape, order="F"))


WIDTH_EDGES = [((64, 32, 1), n) for n in (254, 255, 256)] + [((512, 512, 1), n) for n in (65535, 65536)]


@pytest.mark.parametrize("make", [isolated_voxels, stripes])
@pytest.mark.parametrize("shape,n", WIDTH_EDGES)
def test_width_edges_of_the_section_writer(checker, make, shape, n):
  """Stored width and key width on both sides of 1 -> 2 and 2 -> 4 bytes: n components with a zero
  label (n + 1 values) and without (n values)."""
  vol = make(shape, n)
  binary = checker.compress(vol)
  ccl, ids = _ids(checker, vol, 6)
  assert int(ccl.max()) == n and bool((ccl == 0).any()) == (make is isolated_voxels)
  out = operations.relabel_components(binary, ids)
  _check(checker, binary, out, ccl, ids.size)
  ref = checker.compress(ccl)
  assert crackle_amd.header(ref).crack_format == crackle_amd.header(binary).crack_format
  assert out == ref


def test_general_ids_are_keyed_against_their_sorted_values(checker):
  """Any values below 2^32, not only 0 .. N: the unique list is their ascending set."""
  binary = golden()["c0_voronoi_u8"]
  vol = _volume(checker, binary)
  cc2d, per, total = checker.connected_components(vol)
  ids = np.arange(total, dtype=np.uint64)[::-1] * 977 + 5      # sparse, descending along the stream
  out = operations.relabel_components(binary, ids)
  want = np.zeros(vol.shape, np.uint32, order="F")
  at = 0
  for z, n in enumerate(int(v) for v in per):
    c = cc2d[:, :, z].astype(np.int64)
    want[:, :, z] = ids[at + c - c.min()]
    at += n
  assert np.array_equal(_volume(checker, out), want)
  assert out == checker.compress(want)


def test_empty_volumes(checker):
  for name in ("empty_000", "empty_503"):
    binary = golden()[name]
    h = crackle_amd.header(binary)
    out = operations.relabel_components(binary, np.zeros(0, np.uint64))
    assert out == checker.compress(np.zeros((h.sx, h.sy, h.sz), np.uint32, order="F"), markov_model_order=h.markov_model_order)


def test_bad_arguments(checker):
  binary = golden()["c0_voronoi_u8"]
  _, ids = _ids(checker, _volume(checker, binary), 26)
  for bad in (ids[:-1], np.append(ids, 1), np.zeros(0, np.uint64)):
    with pytest.raises(ValueError, match=rf"{bad.size} ids for the stream's {ids.size} components"):
      operations.relabel_components(binary, bad)
  over = ids.copy()
  over[3] = 2**32
  with pytest.raises(ValueError, match=r"component ids must lie in 0 \.\. 2\^32 - 1"):
    operations.relabel_components(binary, over)
  import os
  with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "v0.npz")) as z:
    v0 = z[[k for k in z.files if "." not in k][0]].tobytes()
  assert crackle_amd.header(v0).format_version == 0
  with pytest.raises(ValueError, match="version 0 has no crack crcs"):
    operations.relabel_components(v0, ids)


def test_python_argument_errors_need_no_device():
  binary = golden()["c0_voronoi_u8"]
  with pytest.raises(ValueError, match="connectivity must be 6, 18 or 26"):
    crackle_amd.connected_components(binary, connectivity=4)
  with pytest.raises(ValueError, match="binary_image=True is not supported"):
    crackle_amd.connected_components(binary, binary_image=True)


def test_restatement_on_hand_made_volumes():
  """Two voxels that touch at a corner only, in-plane and across z; numbering by first voxel."""
  vol = np.zeros((3, 3, 2), np.int16, order="F")
  vol[0, 0, 0] = -4
  vol[1, 1, 0] = -4      # in-plane diagonal: an edge neighbour
  vol[2, 2, 1] = -4      # corner neighbour of (1, 1, 0)
  vol[2, 0, 0] = 6
  for conn, want in ((6, [1, 3, 4]), (18, [1, 1, 3]), (26, [1, 1, 1])):
    ccl, mapping = cc3d_numpy.connected_components(vol, conn)
    assert [int(ccl[0, 0, 0]), int(ccl[1, 1, 0]), int(ccl[2, 2, 1])] == want
    assert int(ccl[2, 0, 0]) == 2 and mapping[2] == 6 and mapping[1] == -4
    assert ccl.dtype == np.uint32 and sorted(mapping) == list(range(1, int(ccl.max()) + 1))
