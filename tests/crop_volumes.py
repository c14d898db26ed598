"""Volumes and boxes for crackle_amd.crop, crop_boxes and chunks, shared by the CPU test that pins what they are
(tests/test_crop_cpu.py) and the GPU tests that run the kernels on them (tests/test_gpu_crop.py).  Plain numpy on top of
tests/erode_volumes.py and tests/recompress_volumes.py.  A box is (x0, x1, y0, y1, z0, z1); each group says what it
aims at."""
import numpy as np

import erode_volumes

HIGH, TOP = (1 << 32) + 5, 2**64 - 1


def voronoi(shape, order="F", **kw):
  kw.setdefault("cell", (4, 4, 2))
  return erode_volumes.voronoi(shape, order, **kw)


def _grid(shape):
  return np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing="ij")


# ---- word edges --------------------------------------------------------------------------------------------------------
# The funnel shift of k_crop_cuts and the run of a word's first pixel in k_crop_labels: a box that begins on a break, one
# column after a break and one column before one; a break at bit 31 with the next at bit 0; a box whose last input word
# has no right neighbour (it ends where the input's rows end).
EDGE_SX = (33, 64, 65, 97)
EDGE_SYZ = 3
EDGE_COLS = (1, 31, 32, 33, 62, 63, 64, 65, 95, 96)      # where the rows change their label (those inside the row)
EDGE_X0 = (0, 1, 31, 32, 33, 63, 64)
EDGE_WIDTHS = (1, 2, 31, 32, 33, 64, 65)


def edge_cols(sx):
  return tuple(c for c in EDGE_COLS if 0 < c < sx)


def edges(sx):
  """uint8, (sx, 3, 3): the k-th stretch of row (y, z) carries 2 + k + 13 ((y + 2 z) % 3): the label changes at every one
  of the columns, and with y and z."""
  x, y, z = _grid((sx, EDGE_SYZ, EDGE_SYZ))
  k = np.searchsorted(edge_cols(sx), x, side="right")
  return np.asfortranarray((2 + k + 13 * ((y + 2 * z) % 3)).astype(np.uint8))


def edge_boxes(sx):
  """Every x0 with every width that fits, times y0 in (0, 1), times z0 in (0, 1); the boxes reach the far faces in y, z."""
  return [(x0, x0 + w, y0, EDGE_SYZ, z0, EDGE_SYZ)
          for x0 in EDGE_X0 for w in EDGE_WIDTHS if x0 + w <= sx for y0 in (0, 1) for z0 in (0, 1)]


def edge_diagonal(sx):
  """A subset that crop() takes one by one: every fifth box of the grid."""
  return edge_boxes(sx)[::5]


# ---- carried labels ----------------------------------------------------------------------------------------------------
# A row without a break from column 3 to column 99: a box that begins in its second or third word takes its first label
# from a run that started two words back.
CARRIED_SHAPE = (130, 3, 2)
CARRIED_BREAKS = (3, 100)
CARRIED_BOXES = [(37, 130, 0, 3, 0, 2), (40, 72, 1, 3, 0, 2), (64, 130, 0, 3, 1, 2), (70, 99, 0, 2, 0, 2), (70, 101, 0, 3, 0, 1), (95, 101, 1, 2, 1, 2)]


def carried():
  x, y, z = _grid(CARRIED_SHAPE)
  k = np.searchsorted(CARRIED_BREAKS, x, side="right")
  return np.asfortranarray((1 + 10 * k + y + 3 * z).astype(np.uint8))


# ---- hand-built rows ---------------------------------------------------------------------------------------------------
# name, dtype, the row, and the literal rows of the crops that begin HAND_OFFSETS columns into it
HAND_OFFSETS = (0, 1, 3)      # from the row's start, from inside its first run, and (placed at 27) across the first word's end
HAND = [
  ("steps", np.uint8, (1, 1, 2, 2, 3, 3, 0, 0, 4, 4),
   ((1, 1, 2, 2, 3, 3, 0, 0, 4, 4), (1, 2, 2, 3, 3, 0, 0, 4, 4), (2, 3, 3, 0, 0, 4, 4))),
  ("wide", np.uint64, (HIGH, HIGH, 7, 7, TOP, TOP, TOP, 3),
   ((HIGH, HIGH, 7, 7, TOP, TOP, TOP, 3), (HIGH, 7, 7, TOP, TOP, TOP, 3), (7, TOP, TOP, TOP, 3))),
  ("one-pixel-runs", np.uint16, (300, 300, 301, 302, 303, 304, 305),
   ((300, 300, 301, 302, 303, 304, 305), (300, 301, 302, 303, 304, 305), (302, 303, 304, 305))),
  ("into-the-background", np.uint8, (9, 9, 9, 77, 77, 8, 8),      # the row's middle equals the label around it
   ((9, 9, 9, 77, 77, 8, 8), (9, 9, 77, 77, 8, 8), (77, 77, 8, 8))),
]
HAND_PLACES = (0, 27, 64)      # x of the row's first pixel: inside the first word, across the first word's end, at the third word's start
HAND_BACKGROUND = 77


def hand(dtype, row, x0):
  """The row at (x0, 1, 0) of a volume of HAND_BACKGROUND that ends where the row ends."""
  vol = np.full((x0 + len(row), 3, 2), HAND_BACKGROUND, dtype, order="F")
  vol[x0:, 1, 0] = row
  return vol


def hand_box(row, x0, offset):
  """From `offset` columns into the row to its end, with the row as the box's first row and slice."""
  return (x0 + offset, x0 + len(row), 1, 3, 0, 2)


# ---- first row and first slice -----------------------------------------------------------------------------------------
# A label boundary exactly at y = 3 and at z = 2: a box with y0 = 3 or z0 = 2 has a first row (slice) that differs from
# the input row (slice) before it.  H at the box's y = 0 and the wrap-around pairs must be the box's own.
FIRST_SHAPE = (70, 8, 5)
FIRST_Y, FIRST_Z = 3, 2
FIRST_BOXES = [(10, 60, 3, 8, 2, 5), (20, 50, 3, 7, 2, 4), (0, 70, 3, 8, 0, 5), (0, 70, 0, 8, 2, 5), (19, 51, 2, 6, 1, 4), (20, 21, 3, 8, 2, 5)]


def first_rows():
  x, y, z = _grid(FIRST_SHAPE)
  lab = 1 + (x >= 20) + 2 * (y >= FIRST_Y) + 4 * (z >= FIRST_Z) + 8 * ((x >= 50) & (y % 2 == 1))
  return np.asfortranarray(lab.astype(np.uint8))


# ---- label counts ------------------------------------------------------------------------------------------------------
# uint16, the 320 labels 0 .. 319 along x: the box [0, n) holds exactly n of them, the largest n - 1.  256 labels: keys
# and stored labels of one byte; 257: two bytes each.  The input's largest label, 319, is in none of the boxes.
COUNTS = (255, 256, 257)
COUNT_SHAPE = (330, 3, 2)


def counted():
  x, _, _ = _grid(COUNT_SHAPE)
  return np.asfortranarray(np.minimum(x, 319).astype(np.uint16))


def count_box(n):
  return (0, n, 1, 3, 0, 2)


# ---- the crack format --------------------------------------------------------------------------------------------------
# The box selects its own crack format: a PERMISSIBLE input (most of it changes its label at every pixel) with an
# IMPERMISSIBLE box (its smooth end), and the reverse.
FORMAT_SHAPE = (96, 24, 4)
FORMAT_SPLIT = 80
FORMAT_BOXES = [(80, 96, 0, 24, 0, 4), (81, 96, 1, 23, 1, 4)]


def format_flip(busy_first):
  """busy_first: the columns below FORMAT_SPLIT change their label at every pixel and the rest is two smooth blocks; or
  the other way round."""
  x, y, z = _grid(FORMAT_SHAPE)
  busy = 1 + (x + 2 * y + 3 * z) % 5
  smooth = 9 + (y >= 12)
  return np.asfortranarray(np.where((x < FORMAT_SPLIT) == busy_first, busy, smooth).astype(np.uint8))


# ---- data widths -------------------------------------------------------------------------------------------------------
WIDTH_SHAPE = (67, 45, 6)
WIDTH_BOX = (5, 60, 3, 40, 1, 5)


def for_dtype(dtype):
  """uint64: labels above 2^32 and 2^64 - 1, inside the box as well."""
  k = voronoi(WIDTH_SHAPE, dtype=np.uint32, seed=43, cell=(8, 8, 3))
  if np.dtype(dtype) != np.uint64:
    return np.asfortranarray(k.astype(dtype))
  wide = k.astype(np.uint64)
  return np.asfortranarray(np.where(wide % 3 == 1, np.uint64(TOP), np.where(wide == 0, np.uint64(0), np.uint64(HIGH) + wide)).astype(np.uint64))


# ---- generated ---------------------------------------------------------------------------------------------------------
GENERATED = [((70, 50, 13), "F", (7, 58, 5, 44, 2, 11)), ((97, 61, 12), "C", (33, 97, 1, 50, 3, 12))]


def generated(i):
  shape, order, box = GENERATED[i]
  return voronoi(shape, order), box


# ---- many words, the encoder's label paths ----------------------------------------------------------------------------
MANY_WORDS_SHAPE = (200, 70, 5)
MANY_WORDS_BOX = (17, 180, 4, 66, 1, 4)      # 163 x 62 x 3: plane_words = 6 * 62, two workgroups of output words per slice


def many_words():
  return voronoi(MANY_WORDS_SHAPE), MANY_WORDS_BOX


STRIP_BOX = (19, 339, 7, 295, 1, 6)      # the shape of erode_volumes.strip_path()


def strip_path():
  """A box of erode_volumes.strip_path()'s shape (large enough for the encoder's strip kernels) out of a larger volume
  of the same cells."""
  return erode_volumes.voronoi((352, 300, 6), "F", seed=32, cell=(32, 32, 4), modulus=13, zero_every=0), STRIP_BOX


RUN_BOX = (37, 32837, 0, 3, 0, 2)


def run_pipeline():
  """Rows of 32800 pixels out of rows of 32900: wider than a strip, the encoder's run pipeline."""
  return erode_volumes.voronoi((32900, 3, 2), "F", dtype=np.uint8, seed=33, cell=(64, 3, 2), modulus=5, zero_every=0), RUN_BOX


# ---- boxes of unequal shapes and z-ranges in one call -------------------------------------------------------------------
# not sorted, with a duplicate and an empty box among them (of generated(0)'s volume)
MIXED_BOXES = [(40, 70, 10, 50, 9, 13), (0, 33, 0, 17, 0, 2), (7, 58, 5, 44, 2, 11), (12, 12, 0, 50, 0, 13), (0, 33, 0, 17, 0, 2), (1, 2, 3, 4, 5, 6), (0, 70, 0, 50, 4, 5)]
