"""Volumes for crackle_amd.erode, shared by the CPU test that pins what they are (tests/test_erode_cpu.py) and the GPU
tests that run the kernels on them (tests/test_gpu_erode.py).  Plain numpy on top of crackle_amd.synth."""
import itertools

import numpy as np

from crackle_amd import synth

CONNECTIVITIES = (6, 18, 26)
NEIGHBOURS = [o for o in itertools.product((-1, 0, 1), repeat=3) if any(o)]      # the 26 positions around a voxel


# ---- which neighbour counts --------------------------------------------------------------------------------------------
PROBE_CENTRE = (4, 4, 4)


def probe(offset, dtype=np.uint8):
  """A 5 x 5 x 5 block of label 1 inset in a 9 x 9 x 9 volume of label 2, with one voxel of label 3 at `offset` from
  the block's centre."""
  vol = np.full((9, 9, 9), 2, dtype, order="F")
  vol[2:7, 2:7, 2:7] = 1
  vol[tuple(c + o for c, o in zip(PROBE_CENTRE, offset))] = 3
  return vol


def probe_centre_survives(offset, connectivity):
  """Stated literally: a face neighbour counts at 6, 18 and 26, an edge-diagonal one at 18 and 26, a corner-diagonal
  one at 26 alone."""
  kind = sum(map(abs, offset))
  return {1: {6: False, 18: False, 26: False}, 2: {6: True, 18: False, 26: False}, 3: {6: True, 18: True, 26: False}}[kind][connectivity]


# ---- word and row edges ------------------------------------------------------------------------------------------------
EDGE_SX = (1, 2, 3, 31, 32, 33, 64, 65)
EDGE_SYZ = (1, 2, 3, 4)
EDGE_VARIANTS = ("columns", "row-tail", "slices")


def edges(shape, variant):
  """Label 5 for x < 32, 6 for 32 <= x < 64, 5 again from x = 64: boundaries at x = 31|32 and 63|64, and a last pixel
  of a row that equals the first of the next (sx <= 32 and sx = 65) or differs from it (sx = 33, 64).
  row-tail: the last row of slice 0 carries label 9 from x = sx // 2 on, so that the row before it ends, and the next
  slice begins, with another label than it has.  slices: slice z carries the labels 10 * z + 5 and 10 * z + 6, so that
  the last pixel of a slice differs from the first of the next, and nothing has an equal neighbour in z."""
  sx, sy, sz = shape
  x = np.arange(sx)
  row = np.where((x >= 32) & (x < 64), 6, 5).astype(np.uint8)
  vol = np.empty(shape, np.uint8, order="F")
  vol[:, :, :] = row[:, None, None]
  if variant == "row-tail":
    vol[sx // 2:, sy - 1, 0] = 9
  elif variant == "slices":
    vol += (10 * np.arange(sz, dtype=np.uint8))[None, None, :]
  else:
    assert variant == "columns"
  return vol


def stripes_y(shape):
  """Rows in bands of three with the labels 1 and 2 in turn, the same in every column and slice.  Without the border
  rule one row of a band survives (two of the first band): in a volume one pixel wide all pairs of lib::pixel_pairs
  are wrap-arounds, and they are few enough for the PERMISSIBLE crack format."""
  vol = np.empty(shape, np.uint8, order="F")
  vol[:, :, :] = (1 + (np.arange(shape[1]) // 3) % 2).astype(np.uint8)[None, :, None]
  return vol


FORMAT_CASES = [("stripes", (1, 36, 4)), ("stripes", (3, 36, 2)), ("single", (1, 6, 5)), ("columns", (64, 3, 4)), ("row-tail", (33, 4, 3)), ("slices", (65, 3, 3))]


def format_case(kind, shape):
  if kind == "single":
    return single_label(shape, dtype=np.uint8)
  return stripes_y(shape) if kind == "stripes" else edges(shape, kind)


# ---- the border rule ---------------------------------------------------------------------------------------------------
def single_label(shape=(37, 6, 5), label=7, dtype=np.uint16):
  return np.full(shape, label, dtype, order="F")


SLAB_SHAPE = (40, 11, 9)


def slab(axis, thickness, dtype=np.uint8):
  """Label 2 everywhere but a slab of label 4, `thickness` voxels thick along `axis`, from position 3 on (the slab
  reaches the faces of the volume along the other two axes)."""
  vol = np.full(SLAB_SHAPE, 2, dtype, order="F")
  at = [slice(None)] * 3
  at[axis] = slice(3, 3 + thickness)
  vol[tuple(at)] = 4
  return vol


# ---- nothing survives --------------------------------------------------------------------------------------------------
def thin_sheets(shape=(70, 9, 5), dtype=np.uint16):
  """Sheets two voxels thick in x with the labels 1, 2, 3, 1, ... (the first and the last one voxel thick, so that
  they go without the border rule as well): every voxel has a neighbour of another label."""
  assert shape[0] % 2 == 0
  x = np.arange(shape[0])
  vol = np.empty(shape, dtype, order="F")
  vol[:, :, :] = (1 + ((x + 1) // 2) % 3).astype(dtype)[:, None, None]
  return vol


WIDE = 1 << 40


def wide_label_on_a_sheet():
  """uint64: label 2^40 on a sheet two voxels thick between thick blocks of the labels 3 and 4.  The sheet goes, and
  with it the only label that needs more than one byte."""
  vol = np.full((41, 12, 8), 3, np.uint64, order="F")
  vol[20:, :, :] = 4
  vol[18:20, :, :] = WIDE
  return vol


def high_bits_only():
  """uint64: two thick blocks whose labels differ above bit 32 alone."""
  vol = np.full((40, 10, 8), (1 << 32) + 5, np.uint64, order="F")
  vol[:, 5:, :] = (2 << 32) + 5
  return vol


# ---- generated ---------------------------------------------------------------------------------------------------------
def voronoi(shape, order="F", dtype=np.uint32, seed=41, cell=(16, 16, 6), modulus=40, offset=0, zero_every=5):
  """Compact cells whose labels recur; every label that is a multiple of zero_every (before the offset) is background."""
  lab = synth.as_numpy_f(synth.voronoi_labels(shape, dtype, seed=seed, cell=cell, modulus=modulus, offset=offset)).copy(order="F")
  if zero_every:
    lab[(lab - lab.dtype.type(offset)) % lab.dtype.type(zero_every) == 0] = 0
  return np.ascontiguousarray(lab) if order == "C" else lab


GENERATED = [((70, 50, 13), "F"), ((97, 61, 12), "C")]


MERGE = {7: 3, 9: 3}


def merging():
  """Few labels, so that cells of the labels 3, 7 and 9 touch: remapped by MERGE their boundaries are false ones."""
  return voronoi(GENERATED[0][0], "F", modulus=12)


def merged(vol):
  return np.where(np.isin(vol, list(MERGE)), vol.dtype.type(3), vol).astype(vol.dtype, order="F")


def for_dtype(dtype):
  offset = WIDE if np.dtype(dtype) == np.uint64 else 0
  return voronoi((67, 45, 12), "F", dtype=dtype, seed=43, modulus=40, offset=offset)


def strip_path():
  """Large enough for the encoder's strip kernels (tests/test_gpu_recompress.py: test_strip_path_and_its_hand_over)."""
  return voronoi((320, 288, 5), "F", seed=32, cell=(32, 32, 4), modulus=13, zero_every=0)


def run_pipeline():
  """Rows wider than a strip: the encoder's run pipeline (tests/test_gpu_recompress.py: test_rows_wider_than_a_strip).
  Three rows and two slices: eroded without the border rule only."""
  return voronoi((32800, 3, 2), "F", dtype=np.uint8, seed=33, cell=(64, 3, 2), modulus=5, zero_every=0)


def survival(vol, eroded):
  """Fraction of the nonzero voxels that keep their label, and the nonzero labels left."""
  return np.count_nonzero(eroded) / max(1, np.count_nonzero(vol)), np.unique(eroded[eroded != 0]).size
