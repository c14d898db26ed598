"""Volumes for crackle_amd.downsample, shared by the CPU test that pins what they are (tests/test_downsample_cpu.py) and
the GPU tests that run the kernels on them (tests/test_gpu_downsample.py).  Plain numpy on top of tests/erode_volumes.py."""
import numpy as np

import erode_volumes
from dilate_volumes import rows      # (row y carries pattern[y % len(pattern)])

FACTORS = ((2, 2, 1), (2, 2, 2))
HIGH_1, HIGH_2, TOP = (1 << 32) + 5, (2 << 32) + 5, 2**64 - 1


# ---- generated ---------------------------------------------------------------------------------------------------------
GENERATED = [((70, 50, 13), "F", dict()), ((97, 61, 12), "C", dict(modulus=251, zero_every=0))]


def voronoi(shape, order="F", **kw):
  """Cells of about 4 x 4 x 2 voxels: most 2 x 2 blocks are cut by a cell face."""
  kw.setdefault("cell", (4, 4, 2))
  return erode_volumes.voronoi(shape, order, **kw)


def generated(i):
  shape, order, kw = GENERATED[i]
  return voronoi(shape, order, **kw)


# ---- hand-built blocks -------------------------------------------------------------------------------------------------
# name, dtype, (a, b, c, d) at (x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1), the literal answer of the reference's rule
BLOCKS_221 = [
  ("a-eq-b", np.uint8, (1, 1, 2, 3), 1),
  ("a-eq-c", np.uint8, (1, 2, 1, 3), 1),
  ("b-eq-c", np.uint8, (1, 2, 2, 1), 2),
  ("else-d", np.uint8, (1, 2, 3, 4), 4),
  ("else-d-eq-b", np.uint8, (1, 2, 3, 2), 2),
  ("zero-is-a-label", np.uint8, (0, 0, 7, 7), 0),
  ("high-bits", np.uint64, (HIGH_1, HIGH_2, HIGH_2, HIGH_1), HIGH_2),
]
# name, dtype, the eight voxels x fastest, then y, then z, the literal answer of "most often, ties to the smallest"
BLOCKS_222 = [
  ("3-3-2", np.uint8, (7, 5, 7, 5, 2, 7, 5, 2), 5),
  ("4-4-tie", np.uint8, (9, 9, 9, 9, 4, 4, 4, 4), 4),
  ("2-2-2-2-tie", np.uint8, (8, 6, 8, 6, 3, 7, 7, 3), 3),
  ("eight-different", np.uint8, (18, 17, 16, 15, 14, 13, 12, 11), 11),
  ("5-3", np.uint8, (2, 9, 9, 2, 9, 9, 2, 9), 9),
  ("zero-is-a-label", np.uint8, (0, 6, 0, 6, 0, 6, 0, 6), 0),
  ("high-bits-tie", np.uint64, (HIGH_2, HIGH_1, HIGH_2, HIGH_1, HIGH_1, HIGH_2, HIGH_1, HIGH_2), HIGH_1),
  ("high-bits-majority", np.uint64, (HIGH_2, HIGH_1, HIGH_2, HIGH_1, HIGH_2, HIGH_2, HIGH_1, HIGH_2), HIGH_2),
  ("top-bit-tie", np.uint64, (TOP, 3, TOP, 3, 3, TOP, 3, TOP), 3),
  ("top-bit-majority", np.uint64, (TOP, 3, TOP, TOP, 3, TOP, 3, TOP), TOP),
]
# partial blocks: shape of what exists, its voxels x fastest, the answers of (2, 2, 1) per slice and of (2, 2, 2)
PARTIAL = [
  ("four", (2, 2, 1), (1, 2, 2, 1), (2,), 1),
  ("two-in-x", (2, 1, 1), (5, 3), (5,), 3),
  ("two-in-y", (1, 2, 1), (5, 3), (5,), 3),
  ("two-in-z", (1, 1, 2), (5, 3), (5, 3), 3),
  ("one", (1, 1, 1), (7,), (7,), 7),
  ("four-in-xz", (2, 1, 2), (6, 2, 9, 6), (6, 9), 6),
  ("four-in-yz", (1, 2, 2), (4, 8, 8, 3), (4, 8), 8),
]
BACKGROUND = 100
PLACES = (0, 62, 64)      # input x of the block: bit 0 and bit 31 of the first output word, bit 0 of the second


def block(dtype, values, shape=(2, 2, 2)):
  return np.array(values, dtype).reshape(shape, order="F")


def place(blk, x0, y0=2):
  """The block at (x0, y0, 0) of a volume of BACKGROUND that ends where the block ends, so a partial block is one."""
  bx, by, bz = blk.shape
  vol = np.full((x0 + bx, y0 + by, bz), BACKGROUND, blk.dtype, order="F")
  vol[x0:, y0:, :] = blk
  return vol


# ---- word and row edges ------------------------------------------------------------------------------------------------
EDGE_SX = (1, 2, 3, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129)
EDGE_SYZ = (1, 2, 3, 4)
EDGE_VARIANTS = ("breaks", "one-pixel-labels", "wrap-pairs", "uniform")
EDGE_COLUMNS = (1, 62, 63, 64, 65)


def edges(shape, variant):
  """breaks: the label changes at the input columns 1, 62, 63, 64, 65 and sx - 1 (and every row begins at 0), and with
      y and z in a period of three, so that blocks are not uniform in y and z either.
  one-pixel-labels: every pixel differs from its neighbours in x: a cut at every output pixel.
  wrap-pairs: the first two and the last two columns carry label 9, so that the last pooled pixel of a row equals the first
      of the next row, and the last of a slice the first of the next slice.
  uniform: one label, no cuts."""
  sx, sy, sz = shape
  x, y, z = np.meshgrid(np.arange(sx), np.arange(sy), np.arange(sz), indexing="ij")
  if variant == "breaks":
    cols = sorted(set(c for c in EDGE_COLUMNS + (sx - 1,) if 0 < c < sx))
    vol = 2 + np.searchsorted(cols, x, side="right") + 7 * ((y + 2 * z) % 3)
  elif variant == "one-pixel-labels":
    vol = 1 + (x + 3 * y + 5 * z) % 251
  elif variant == "wrap-pairs":
    vol = np.where((x < 2) | (x >= sx - 2), 9, 3 + (x // 3 + y // 2 + z) % 2)
  else:
    assert variant == "uniform"
    vol = np.full(shape, 4)
  return np.asfortranarray(vol.astype(np.uint8))


# ---- the crack format --------------------------------------------------------------------------------------------------
MIXED_SHAPE = (66, 10, 4)


def mixed_formats(seed=7):
  """Even slices of one label, odd slices of three-label noise: pooled 2 x 2 x 1, the slices pick different crack formats."""
  rng = np.random.default_rng(seed)
  vol = np.full(MIXED_SHAPE, 2, np.uint8, order="F")
  vol[:, :, 1::2] = rng.integers(1, 4, (MIXED_SHAPE[0], MIXED_SHAPE[1], MIXED_SHAPE[2] // 2))
  return vol


# name, the rows' pattern, PERMISSIBLE before, PERMISSIBLE after (both factors)
FORMAT_CASES = [("1-2-1-3", (1, 2, 1, 3), True, False), ("1-1-2-2", (1, 1, 2, 2), False, True)]


# ---- labels that vanish ------------------------------------------------------------------------------------------------
def lonely_labels(shape=(50, 30, 2)):
  """uint16: background 5, and at position d (x and y odd) of every block of slice 0 a label of its own, 1000 and up:
  more than 300 labels that occur once and lose in their block under both rules."""
  vol = np.full(shape, 5, np.uint16, order="F")
  n = (shape[0] // 2) * (shape[1] // 2)
  vol[1::2, 1::2, 0] = (1000 + np.arange(n)).reshape((shape[0] // 2, shape[1] // 2), order="F")
  return vol


def survivors(n):
  """uint16, 64 x 2 ceil(n / 32) x 2: block k carries label 1 + min(k, n - 1) in seven of its eight voxels and the label
  1000 + k at position d of slice 0: exactly n labels survive either pooling, and the input holds more."""
  nby = -(-n // 32)
  k = np.arange(32)[:, None] + 32 * np.arange(nby)[None, :]
  per_block = (1 + np.minimum(k, n - 1)).astype(np.uint16)
  vol = np.empty((64, 2 * nby, 2), np.uint16, order="F")
  vol[:, :, :] = np.repeat(np.repeat(per_block, 2, axis=0), 2, axis=1)[:, :, None]
  vol[1::2, 1::2, 0] = (1000 + k).astype(np.uint16)
  return vol


# ---- widths, many words, the encoder's label paths ---------------------------------------------------------------------
def for_dtype(dtype):
  offset = erode_volumes.WIDE if np.dtype(dtype) == np.uint64 else 0
  return voronoi((67, 45, 12), "F", dtype=dtype, seed=43, modulus=40, offset=offset)


MANY_WORDS = (194, 200, 6)      # pooled: plane_words = 4 * 100, two workgroups of output words per slice


def strip_path():
  """Pooled, 320 x 288 with cells of about 32 x 32: what tests/erode_volumes.py's strip_path is, large enough for the
  encoder's strip kernels and with few enough crack nodes for them to run beside the trail's walk (smaller cells send the
  encoder to its run pipeline, whatever the size)."""
  return voronoi((640, 576, 5), "F", seed=32, cell=(64, 64, 4), modulus=13, zero_every=0)


def run_pipeline():
  """Pooled, rows of 32800 pixels: wider than a strip, the encoder's run pipeline (tests/erode_volumes.py: run_pipeline)."""
  return voronoi((65600, 6, 2), "F", dtype=np.uint8, seed=33, cell=(64, 3, 2), modulus=5, zero_every=0)
