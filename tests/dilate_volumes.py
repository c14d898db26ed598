"""Volumes for crackle_amd.dilate, shared by the CPU test that pins what they are (tests/test_dilate_cpu.py) and the GPU
tests that run the kernels on them (tests/test_gpu_dilate.py).  Plain numpy on top of tests/erode_volumes.py."""
import numpy as np

import dilate_numpy
import erode_volumes

CONNECTIVITIES = erode_volumes.CONNECTIVITIES
NEIGHBOURS = erode_volumes.NEIGHBOURS
voronoi = erode_volumes.voronoi
GENERATED = erode_volumes.GENERATED


# ---- which neighbour counts --------------------------------------------------------------------------------------------
PROBE_CENTRE = (4, 4, 4)


def probe(offset, dtype=np.uint8):
  """A 9 x 9 x 9 volume of zeros with one voxel of label 3 at `offset` from the centre."""
  vol = np.zeros((9, 9, 9), dtype, order="F")
  vol[tuple(c + o for c, o in zip(PROBE_CENTRE, offset))] = 3
  return vol


def probe_centre_gained(offset, connectivity):
  """Stated literally: a face neighbour counts at 6, 18 and 26, an edge-diagonal one at 18 and 26, a corner-diagonal
  one at 26 alone."""
  kind = sum(map(abs, offset))
  return {1: {6: True, 18: True, 26: True}, 2: {6: False, 18: True, 26: True}, 3: {6: False, 18: False, 26: True}}[kind][connectivity]


# ---- the mode and the tie rule -----------------------------------------------------------------------------------------
HIGH_1, HIGH_2, TOP = (1 << 32) + 5, (2 << 32) + 5, 2**64 - 1
X, Y, Z = (1, 0, 0), (0, 1, 0), (0, 0, 1)
# name, dtype, {offset from the centre: label}, the centre's label at connectivity 6, 18, 26
MODE_CASES = [
  ("two-against-one", np.uint8, {X: 9, (-1, 0, 0): 9, Y: 2}, (9, 9, 9)),
  ("one-against-one", np.uint8, {X: 9, Y: 2}, (2, 2, 2)),
  ("one-against-one-swapped", np.uint8, {X: 2, Y: 9}, (2, 2, 2)),
  ("three-way-tie", np.uint8, {X: 7, Y: 4, Z: 11}, (4, 4, 4)),
  ("high-bits-tie", np.uint64, {X: HIGH_2, Y: HIGH_1}, (HIGH_1, HIGH_1, HIGH_1)),
  ("high-bits-majority", np.uint64, {X: HIGH_2, Y: HIGH_1, Z: HIGH_2}, (HIGH_2, HIGH_2, HIGH_2)),
  ("top-bit-tie", np.uint64, {X: TOP, Y: 3}, (3, 3, 3)),
  ("top-bit-majority", np.uint64, {X: TOP, Y: 3, (0, 0, -1): TOP}, (TOP, TOP, TOP)),
  # one face neighbour, two edge neighbours, three corner neighbours: another winner at every connectivity
  ("face-edge-corner", np.uint8, {X: 5, (1, 1, 0): 3, (1, -1, 0): 3, (1, 1, 1): 8, (-1, 1, 1): 8, (1, -1, -1): 8}, (5, 3, 8)),
  # the edge neighbours only tie with the face neighbours' label, the corners decide
  ("corners-break-the-tie", np.uint8, {X: 6, Y: 6, (1, 1, 0): 2, (0, 1, 1): 2, (1, 1, 1): 6}, (6, 2, 6)),
]


def mode_case(dtype, entries):
  """A 7 x 7 x 7 volume of zeros with the given labels around its centre (3, 3, 3)."""
  vol = np.zeros((7, 7, 7), dtype, order="F")
  for off, label in entries.items():
    vol[tuple(3 + o for o in off)] = label
  return vol


MODE_CENTRE = (3, 3, 3)


# ---- word and row edges ------------------------------------------------------------------------------------------------
EDGE_SX = erode_volumes.EDGE_SX
EDGE_SYZ = erode_volumes.EDGE_SYZ
EDGE_VARIANTS = ("columns", "tail-label", "tail-background", "all-gained", "one-pixel-labels")
EDGE_COLUMNS = (0, 31, 32, 63, 64)


def edges(shape, variant):
  """columns: background columns at x = 0, 31, 32, 63, 64 and sx - 1; the stretches between them carry the labels
      2, 3, 4, ..., ten more where y + z is odd, so that a background pixel sees other labels beside, above and below.
  tail-label: every row begins with two background pixels and ends in a label (3 + y % 3): the first pixel of a row
      has no labelled neighbour, but the pixel before it in x-fastest order, the end of the row above, is labelled.
  tail-background: the reverse, every row ends in two background pixels and begins with a label.
  all-gained: the odd rows are background, the even rows carry label 4 + z: with sy >= 2 every pixel of an odd row is
      gained, so whole words are.
  one-pixel-labels: the odd rows are background, the even rows carry the labels x + 1 + y, one pixel each."""
  sx, sy, sz = shape
  x, y, z = np.meshgrid(np.arange(sx), np.arange(sy), np.arange(sz), indexing="ij")
  if variant == "columns":
    cols = sorted(set(c for c in EDGE_COLUMNS + (sx - 1,) if c < sx))
    vol = 2 + np.searchsorted(cols, x, side="left") + 10 * ((y + z) % 2)
    vol[np.isin(x, cols)] = 0
  elif variant == "tail-label":
    vol = np.where(x < 2, 0, 3 + y % 3)
  elif variant == "tail-background":
    vol = np.where(x >= sx - 2, 0, 3 + y % 3)
  elif variant == "all-gained":
    vol = np.where(y % 2 == 1, 0, 4 + z)
  else:
    assert variant == "one-pixel-labels"
    vol = np.where(y % 2 == 1, 0, x + 1 + y)
  return np.asfortranarray(vol.astype(np.uint8))


# ---- the crack format --------------------------------------------------------------------------------------------------
FORMAT_SHAPE = (1, 36, 4)
FORMAT_CASES = [("1-0-2-0", (1, 0, 2, 0)), ("1-2-0-3-4-5", (1, 2, 0, 3, 4, 5))]


def rows(pattern, shape=FORMAT_SHAPE):
  """Row y carries pattern[y % len(pattern)], the same in every column and slice."""
  vol = np.empty(shape, np.uint8, order="F")
  vol[:, :, :] = np.array([pattern[y % len(pattern)] for y in range(shape[1])], np.uint8)[None, :, None]
  return vol


# ---- nothing gained ----------------------------------------------------------------------------------------------------
def no_background(shape=(70, 50, 13)):
  vol = voronoi(shape, "F", zero_every=0) + np.uint32(1)
  return np.asfortranarray(vol)


def single_voxel(shape=(37, 6, 5), at=(17, 3, 2), label=7, dtype=np.uint16):
  vol = np.zeros(shape, dtype, order="F")
  vol[at] = label
  return vol


# ---- generated ---------------------------------------------------------------------------------------------------------
def seams(shape, order="F", **kw):
  """erode_volumes.voronoi (whole cells of background: every fifth label) with every voxel set to 0 whose label
  differs from its +x, +y or +z neighbour: background one voxel wide between the cells."""
  lab = voronoi(shape, "F", **kw)
  cut = np.zeros(lab.shape, bool)
  cut[:-1, :, :] |= lab[:-1, :, :] != lab[1:, :, :]
  cut[:, :-1, :] |= lab[:, :-1, :] != lab[:, 1:, :]
  cut[:, :, :-1] |= lab[:, :, :-1] != lab[:, :, 1:]
  out = np.where(cut, lab.dtype.type(0), lab)
  return np.ascontiguousarray(out) if order == "C" else np.asfortranarray(out)


MANY_WORDS = (97, 100, 12)      # plane_words = 4 * 100: two workgroups of words per slice


def for_dtype(dtype):
  offset = erode_volumes.WIDE if np.dtype(dtype) == np.uint64 else 0
  return seams((67, 45, 12), "F", dtype=dtype, seed=43, modulus=40, offset=offset)


def _a_fifth_zeroed(vol):
  out = vol.copy(order="F")
  out[out % out.dtype.type(5) == 0] = 0
  return out


def strip_path():
  return _a_fifth_zeroed(erode_volumes.strip_path())


def run_pipeline():
  return _a_fifth_zeroed(erode_volumes.run_pipeline())


def pit():
  """A block of label 6 in a background, with a pit of one voxel in the middle of its top face and a hole of one voxel
  inside: closing fills the hole at every connectivity and the pit at 18 and 26 (at 6 the voxel above the pit is not
  gained, so erosion opens the pit again)."""
  vol = np.zeros((20, 12, 9), np.uint8, order="F")
  vol[4:16, 3:9, 2:7] = 6
  vol[10, 5, 6] = 0
  vol[8, 5, 4] = 0
  return vol


def stats(vol, connectivity):
  """Of the gained voxels the share that sees two or more labels (contested), whose most frequent label is not alone
  (tied), whose mode is not the smallest and not the largest label it sees; and the share of the volume that is
  still 0 afterwards."""
  stack = dilate_numpy.neighbour_stack(vol, connectivity)
  best, best_n = dilate_numpy.modes(stack)
  gained = (np.asarray(vol) == 0) & (best_n > 0)
  s = np.sort(stack, axis=0)[:, gained]
  mode, top = best[gained], best_n[gained]
  at_top = np.zeros(mode.shape, np.int64)
  distinct = (s[0] != 0).astype(np.int64)
  for i in range(s.shape[0]):
    n = (s == s[i]).sum(axis=0)
    at_top += (s[i] != 0) & (n == top)
    if i:
      distinct += (s[i] != 0) & (s[i] != s[i - 1])
  big = np.iinfo(s.dtype).max
  smallest = np.where(s != 0, s, big).min(axis=0)
  g = max(1, int(gained.sum()))
  out = dilate_numpy.dilate(vol, connectivity)
  return dict(
    gained=int(gained.sum()), contested=float((distinct >= 2).sum()) / g, tied=float((at_top > top).sum()) / g,
    not_smallest=float((mode != smallest).sum()) / g, not_largest=float((mode != s.max(axis=0)).sum()) / g,
    still_zero=float((out == 0).sum()) / out.size,
  )
