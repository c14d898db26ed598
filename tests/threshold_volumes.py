"""Volumes that sit exactly on the encoder's two whole-volume decisions: the crack format (pixel_pairs against
voxels // 2) and the stored width (the byte width of max_label).  Plain numpy; shared by the CPU test that pins
these constructions against the checker and by the GPU tests that run the kernels on them.

pixel_pairs counts equal neighbours of the F-order flat sequence (x fastest): a row's last voxel pairs with the next
row's first, a slice's last with the next slice's first."""
import numpy as np

DTYPES = (np.uint8, np.uint16, np.uint32, np.uint64)
PERMISSIBLE, IMPERMISSIBLE = 1, 0
FLAT, PINS = 0, 2


def lanes(dtype):
  """P: labels in a 16-byte vector."""
  return 16 // np.dtype(dtype).itemsize


def byte_width(x):
  return 1 if x <= 0xFF else 2 if x <= 0xFFFF else 4 if x <= 0xFFFFFFFF else 8


def flat(arr):
  return np.asarray(arr).reshape(-1, order="F")


def pairs(arr):
  """Equal linear neighbours, wrap-arounds included."""
  f = flat(arr)
  return int(np.count_nonzero(f[1:] == f[:-1]))


def pairs_in_rows(arr):
  """The pairs whose right voxel does not start a row: what a count that forgets the wrap-arounds finds."""
  f = flat(arr)
  sx = arr.shape[0]
  right = np.arange(1, f.size)
  return int(np.count_nonzero((f[1:] == f[:-1]) & (right % sx != 0)))


def wraps_in_rows(arr):
  """pairs - pairs_in_rows: the equal pairs across a row or slice wrap-around."""
  return pairs(arr) - pairs_in_rows(arr)


def pairs_volume(shape, dtype, k, place):
  """A volume of labels {1, 2, 3} with exactly k equal linear neighbours: a base pattern without any (vertical
  stripes for even sx, a checkerboard of the flat index for odd sx) and one stretch of k + 1 voxels of label 3, from
  voxel 0 (place "head") or up to the last voxel ("tail")."""
  sx, sy, sz = (int(s) for s in shape)
  n = sx * sy * sz
  if not 0 <= k < n:
    raise ValueError(f"k = {k} needs {k + 1} voxels, the volume has {n}")
  i = np.arange(n, dtype=np.int64)
  f = (1 + ((i % sx) & 1 if sx % 2 == 0 else i & 1)).astype(dtype)
  if place == "head":
    f[:k + 1] = 3
  elif place == "tail":
    f[n - k - 1:] = 3
  else:
    raise ValueError(place)
  return f.reshape((sx, sy, sz), order="F")


def random_volume(shape, dtype, seed=7):
  """Seeded noise of the labels 0 .. 2: a third of the neighbours are equal."""
  from crackle_amd import synth
  return np.asfortranarray(synth.random_labels(shape, dtype, seed=seed, high=3))


def with_extremes(arr):
  """The volume with the dtype's maximum in its first and its last voxel (both differ from their neighbours: the
  pair count changes by what the two voxels took part in before, which the caller counts again)."""
  f = flat(arr).copy()
  f[0] = f[-1] = np.iinfo(arr.dtype).max
  return f.reshape(arr.shape, order="F")


def max_positions(shape, dtype):
  """name -> (x, y, z) of the places where a strip of 64 P pixels x 32 rows begins, ends or is cut short."""
  sx, sy, sz = shape
  p = lanes(dtype)
  return {
    "first": (0, 0, 0),
    "last": (sx - 1, sy - 1, sz - 1),
    "strip_end": (64 * p - 1, 5, 0),      # last pixel of the full strip
    "strip_next": (64 * p, 5, 0),         # first pixel of the partial strip
    "y31": (3, 31, 0),                    # last row of the full band
    "y32": (3, 32, 0),                    # the one-row band
    "slice1": (0, 0, 1),
  }


POSITIONS = ("first", "last", "strip_end", "strip_next", "y31", "y32", "slice1")


def max_at(shape, dtype, value, position):
  """Labels 1 .. 3 in blocks of 8 x 8 pixels and one voxel of `value` at the named position."""
  sx, sy, sz = (int(s) for s in shape)
  x, y, z = np.meshgrid(np.arange(sx), np.arange(sy), np.arange(sz), indexing="ij")
  arr = np.asfortranarray((1 + (x // 8 + y // 8 + z) % 3).astype(dtype))
  arr[max_positions(shape, dtype)[position]] = value
  return arr


# ---- the cases, shared by the CPU test that pins them and the GPU tests that use them -------------------------------
def strip_shapes(dtype):
  p = lanes(dtype)
  return [(65 * p, 33, 3), (65 * p + 1, 33, 3)]


def small_shapes(dtype):
  p = lanes(dtype)
  return [(p, 1, 1), (p - 1, 2, 2), (17, 3, 1)]


def all_shapes(dtype):
  return strip_shapes(dtype) + small_shapes(dtype)


def threshold_ks(shape):
  """H - 1, H, H + 1 for H = voxels // 2, as far as the volume can hold them (k + 1 voxels)."""
  n = shape[0] * shape[1] * shape[2]
  h = n // 2
  return [k for k in (h - 1, h, h + 1) if 0 <= k < n]


def format_shapes(dtype):
  """The shapes of the format decision: both strip shapes and the odd voxel count."""
  return strip_shapes(dtype) + [(17, 3, 1)]


# (dtype, value, stored width): each width's first value, the widest value, and one control below each threshold
MAX_VALUES = [
  (np.uint16, 256, 2), (np.uint32, 65536, 4), (np.uint64, 1 << 32, 8), (np.uint64, (1 << 64) - 1, 8),
  (np.uint16, 255, 1), (np.uint32, 65535, 2), (np.uint64, (1 << 32) - 1, 4),
]

POOL_WIDTHS = (48, 40)


def pooling_slices(width, dtype):
  """Three slices of width x 5 at H - 1, H, H + 1 pairs, head and tail alternating."""
  shape = (width, 5, 1)
  h = width * 5 // 2
  return [pairs_volume(shape, dtype, k, place)[:, :, 0] for k, place in ((h - 1, "head"), (h, "tail"), (h + 1, "head"))]


def pooling_input(width, dtype):
  """(2 width, 10, 3): every slice doubled along x and y, so that 2 x 2 x 1 mode pooling returns pooling_slices."""
  return np.asfortranarray(np.stack([np.kron(s, np.ones((2, 2), dtype=dtype)) for s in pooling_slices(width, dtype)], axis=2))


SHARDED_SHAPE = (64, 33, 4)


def sharded_volume(k):
  return pairs_volume(SHARDED_SHAPE, np.uint32, k, "tail")
