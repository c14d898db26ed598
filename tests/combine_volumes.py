"""Pairs (A, B) of volumes for crackle_amd.overlay and crackle_amd.mask_by, shared by the CPU test that pins what they are
(tests/test_combine_cpu.py) and the GPU tests that run the kernels on them (tests/test_gpu_combine.py).  Plain numpy on
top of tests/erode_volumes.py.  B holds zeros in every pair that does not say otherwise: label 0 of B is the one special
value of the three rules."""
import numpy as np

import erode_volumes
import recompress_volumes

HIGH, TOP = (1 << 32) + 5, 2**64 - 1


def voronoi(shape, order="F", **kw):
  kw.setdefault("cell", (4, 4, 2))
  return erode_volumes.voronoi(shape, order, **kw)


def second(shape, order="F", dtype=np.uint32, seed=77, cell=(8, 8, 3), **kw):
  """Another segmentation of the shape with every second label 0: about half of its voxels are background."""
  return erode_volumes.voronoi(shape, order, dtype=dtype, seed=seed, cell=cell, zero_every=2, **kw)


# ---- generated ---------------------------------------------------------------------------------------------------------
GENERATED = [((70, 50, 13), "F"), ((97, 61, 12), "C")]


def generated(i):
  shape, order = GENERATED[i]
  return voronoi(shape, order), second(shape, order, offset=100)      # A's labels are below 40, B's from 101


# ---- word and row edges ------------------------------------------------------------------------------------------------
EDGE_SX = (1, 2, 3, 31, 32, 33, 63, 64, 65)
EDGE_SYZ = (1, 2, 3, 4)
# variant: the columns at which A's rows and B's rows change their label (those inside the row; every row begins at 0)
EDGE_BREAKS = {
  "same-column": ((1, 31, 32, 33, 62), (1, 31, 32, 33, 62)),
  "adjacent-columns": ((1, 31, 33, 63), (2, 32, 34, 64)),
  "bit31-bit0": ((31,), (32,)),      # A's at the last bit of the first word, B's at the first bit of the next
  "carried": ((5,), (7,)),           # no break in the second and third words: both labels are carried in, at sx = 65 from two words back
}
EDGE_VARIANTS = tuple(EDGE_BREAKS) + ("b-zero", "b-full", "a-uniform", "one-pixel-labels")


def breaks_of(variant, sx):
  """(A's, B's) columns of change inside a row of sx pixels."""
  a, b = EDGE_BREAKS["same-column" if variant in ("b-zero", "b-full") else "adjacent-columns" if variant == "a-uniform" else variant]
  return tuple(c for c in a if 0 < c < sx), tuple(c for c in b if 0 < c < sx)


def edges(shape, variant):
  """uint8 pairs.  Between its breaks A carries 2 + k + 7 ((y + 2 z) % 3) in its k-th stretch, B carries 50 + k, or 0 where
  (k + y + z) % 3 == 0: both change their label at every one of their breaks, and with y and z.
  b-zero, b-full: A as in same-column, B all 0 or all 9.  a-uniform: A all 4, B as in adjacent-columns.
  one-pixel-labels: every pixel of A differs from its neighbours in x, and B alternates between 0 and a label."""
  sx, sy, sz = shape
  x, y, z = np.meshgrid(np.arange(sx), np.arange(sy), np.arange(sz), indexing="ij")
  if variant == "one-pixel-labels":
    a = 1 + (x + 3 * y + 5 * z) % 251
    b = np.where((x + y + z) % 2 == 1, 100 + x % 7, 0)
  else:
    cols_a, cols_b = breaks_of(variant, sx)
    ka, kb = np.searchsorted(cols_a, x, side="right"), np.searchsorted(cols_b, x, side="right")
    a = 2 + ka + 7 * ((y + 2 * z) % 3)
    b = np.where((kb + y + z) % 3 == 0, 0, 50 + kb)
    if variant == "b-zero":
      b = np.zeros(shape, int)
    elif variant == "b-full":
      b = np.full(shape, 9)
    elif variant == "a-uniform":
      a = np.full(shape, 4)
  return np.asfortranarray(a.astype(np.uint8)), np.asfortranarray(b.astype(np.uint8))


# ---- hand-built rows ---------------------------------------------------------------------------------------------------
# name, dtype of A, dtype of B, A's row, B's row, the literal rows of overlay, mask_by and mask_by(invert=True)
HAND = [
  ("steps", np.uint8, np.uint8,
   (1, 1, 2, 2, 3, 3, 0, 0, 4, 4), (0, 5, 5, 0, 0, 6, 6, 0, 0, 0),
   (1, 5, 5, 2, 3, 6, 6, 0, 4, 4), (0, 1, 2, 0, 0, 3, 0, 0, 0, 0), (1, 0, 0, 2, 3, 0, 0, 0, 4, 4)),
  ("wider-b", np.uint8, np.uint16,
   (200, 200, 7, 7, 7), (0, 1000, 1000, 0, 3),
   (200, 1000, 1000, 7, 3), (0, 200, 7, 0, 7), (200, 0, 0, 7, 0)),
  ("b-hides-all", np.uint16, np.uint8,
   (300, 301, 302, 303), (1, 1, 2, 2),
   (1, 1, 2, 2), (300, 301, 302, 303), (0, 0, 0, 0)),
  ("equal-neighbours", np.uint8, np.uint8,      # cuts at which the combined label does not change
   (5, 5, 6, 6, 6, 6), (0, 0, 0, 9, 8, 0),
   (5, 5, 6, 9, 8, 6), (0, 0, 0, 6, 6, 0), (5, 5, 6, 0, 0, 6)),
]
HAND_PLACES = (0, 27, 64)      # x of the row's first pixel: inside the first word, across the first word's end, at the third word's start
HAND_BACKGROUND = (77, 0)      # A's and B's label around the row


def hand(a_dtype, b_dtype, row_a, row_b, x0):
  """The two rows at (x0, 1, 0) of volumes of HAND_BACKGROUND that end where the rows end."""
  shape = (x0 + len(row_a), 3, 2)
  a, b = np.full(shape, HAND_BACKGROUND[0], a_dtype, order="F"), np.full(shape, HAND_BACKGROUND[1], b_dtype, order="F")
  a[x0:, 1, 0], b[x0:, 1, 0] = row_a, row_b
  return a, b


# ---- data widths -------------------------------------------------------------------------------------------------------
def narrow_and_wide():
  """A uint8, B uint64 with 0, labels above 2^32 and 2^64 - 1."""
  shape = (67, 45, 5)
  a = voronoi(shape, dtype=np.uint8, seed=43)
  k = voronoi(shape, dtype=np.uint32, seed=44, cell=(8, 8, 3), zero_every=0).astype(np.uint64)
  b = np.where(k % 3 == 0, np.uint64(0), np.where(k % 3 == 1, np.uint64(TOP), np.uint64(HIGH) + k))
  return a, np.asfortranarray(b.astype(np.uint64))


def for_dtypes(a_dtype, b_dtype):
  shape = (67, 45, 6)
  off_a = erode_volumes.WIDE if np.dtype(a_dtype) == np.uint64 else 0
  off_b = erode_volumes.WIDE if np.dtype(b_dtype) == np.uint64 else 0
  return voronoi(shape, dtype=a_dtype, seed=43, offset=off_a), second(shape, dtype=b_dtype, offset=off_b)


# ---- the crack format --------------------------------------------------------------------------------------------------
def formats_differ():
  """A is noise (PERMISSIBLE), B is smooth cells (IMPERMISSIBLE)."""
  shape = (66, 30, 4)
  return np.asfortranarray(recompress_volumes.noise(shape, np.uint8, 21, 4) + np.uint8(1)), second(shape, dtype=np.uint8, cell=(16, 16, 4))


def format_flips():
  """Both inputs change their label at every pixel (PERMISSIBLE), and B is 0 in three columns only: mask_by(invert=True)
  leaves three columns of A in a volume of zeros, which is IMPERMISSIBLE; the other two rules stay PERMISSIBLE."""
  shape = (64, 12, 3)
  x, y, _ = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing="ij")
  a = 1 + x % 2
  b = np.where(np.isin(x, (10, 11, 40)), 0, 5 + (x + y) % 2)
  return np.asfortranarray(a.astype(np.uint8)), np.asfortranarray(b.astype(np.uint8))


# ---- label counts ------------------------------------------------------------------------------------------------------
COUNTS = (255, 256, 257)
COUNT_SHAPE = (40, 16, 2)


def survivors(n, rule):
  """uint16 A with the 320 labels 1 + p // 2 over the pixels p = x + 40 y of both slices, and a B under which exactly n
  labels are left (0 included for the two masks); A's largest labels are among those that vanish.
  overlay: B is 0 on A's first 200 labels and carries n - 200 labels of its own, 5000 and up, over the rest of A.
  keep / drop: B (uint8) is a label / is 0 over A's first n - 1 labels and 0 / a label over the rest."""
  sx, sy, sz = COUNT_SHAPE
  p = (np.arange(sx)[:, None] + sx * np.arange(sy)[None, :])[:, :, None] * np.ones((1, 1, sz), int)
  a = (1 + p // 2).astype(np.uint16)
  if rule == "overlay":
    b = np.where(p < 400, 0, 5000 + np.minimum((p - 400) // 2, n - 201)).astype(np.uint16)
  else:
    inside = p < 2 * (n - 1)
    b = np.where(inside == (rule == "keep"), 7, 0).astype(np.uint8)
  return np.asfortranarray(a), np.asfortranarray(b)


# ---- many words, the encoder's label paths ----------------------------------------------------------------------------
MANY_WORDS = (160, 60, 3)      # plane_words = 5 * 60: two workgroups of words per slice


def many_words():
  return voronoi(MANY_WORDS), second(MANY_WORDS)


def strip_path():
  """tests/erode_volumes.py's strip_path (what tests/downsample_volumes.py's is after pooling) under a coarser B: large
  enough for the encoder's strip kernels, with few enough crack nodes for them to run beside the trail's walk."""
  return erode_volumes.strip_path(), second((320, 288, 5), seed=35, cell=(64, 64, 4), modulus=13)


def run_pipeline():
  """Rows of 32800 pixels: wider than a strip, the encoder's run pipeline (tests/erode_volumes.py: run_pipeline)."""
  return erode_volumes.run_pipeline(), second((32800, 3, 2), dtype=np.uint8, seed=34, cell=(128, 3, 2), modulus=5)
