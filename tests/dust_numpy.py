"""A scipy restatement of crackle_amd.dust, computed from the INPUT array (never from what the code under
test decodes), in the manner of tests/cc3d_numpy.py.

For every distinct nonzero label l, scipy.ndimage.label(vol == l, structure) with the 6-, 18- or
26-neighbourhood gives the 3D-connected pieces of that label (binary_image: one call on vol != 0, so a
piece may hold several labels).  np.bincount gives the pieces' sizes; the voxels of a piece with fewer than
`threshold` voxels (invert: with `threshold` or more) become 0, everything else is kept as it is.

Each label is looked at inside its bounding box only (scipy.ndimage.find_objects), which changes nothing but
the time a volume of many labels takes.
"""
from typing import Tuple

import numpy as np
from scipy import ndimage

_RANK = {6: 1, 18: 2, 26: 3}


def _pieces(vol: np.ndarray, connectivity: int, binary_image: bool):
  """Yields (box, piece image of the box, number of pieces): the pieces of one label (or of the foreground) each time."""
  structure = ndimage.generate_binary_structure(3, _RANK[connectivity])
  if binary_image:
    part, n = ndimage.label(vol != 0, structure)
    yield (slice(None),) * 3, part, n
    return
  uniq, inverse = np.unique(vol, return_inverse=True)
  dense = inverse.reshape(vol.shape).astype(np.int32) + (0 if uniq[0] == 0 else 1)      # label 0 -> 0, the others 1 ..
  for i, box in enumerate(ndimage.find_objects(dense)):
    if box is not None:
      part, n = ndimage.label(dense[box] == i + 1, structure)
      yield box, part, n


def dust(vol: np.ndarray, threshold: int, connectivity: int = 26, binary_image: bool = False, invert: bool = False) -> Tuple[np.ndarray, int]:
  """(expected volume: vol's dtype, shape and memory order; number of 3D components set to 0)."""
  vol = np.asarray(vol)
  threshold = min(int(threshold), vol.size + 1)      # (no piece is larger than the volume: the same decisions, in int64)
  out = vol.copy(order="K")
  removed = 0
  for box, part, n in _pieces(vol, connectivity, binary_image):
    sizes = np.bincount(part.ravel(), minlength=n + 1)
    small = sizes < threshold
    drop = ~small if invert else small
    drop[0] = False      # what is not of this label is no piece
    removed += int(np.count_nonzero(drop))
    if drop.any():
      out[box][drop[part]] = 0
  return out, removed


def sizes(vol: np.ndarray, connectivity: int = 26, binary_image: bool = False) -> np.ndarray:
  """The voxel counts of all components, ascending."""
  got = [np.bincount(part.ravel(), minlength=n + 1)[1:] for _, part, n in _pieces(np.asarray(vol), connectivity, binary_image)]
  return np.sort(np.concatenate(got)) if got else np.zeros(0, np.int64)
