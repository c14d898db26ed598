"""A scipy restatement of crackle_amd.fill_holes, computed from the INPUT array (never from what the code under
test decodes), in the manner of tests/dust_numpy.py.

scipy.ndimage.label(vol == 0, structure) with the 6-, 18- or 26-neighbourhood finds the holes, find_objects the box
of each.  A box that reaches a face of the volume means that a voxel of the hole lies on that face: the hole is open
and stays.  Otherwise the hole's mask is taken in its box grown by one voxel on every side (which is inside the
volume then); binary_dilation with the face structure, minus the mask, gives the face neighbours that are not in the
hole, and np.unique the labels there.  Exactly one nonzero label fills the hole with it.  A zero among those labels
(a face neighbour of label 0 outside the hole) cannot occur: face neighbours of label 0 are in the same hole at every
connectivity; it is treated as a second label all the same.
"""
from typing import NamedTuple

import numpy as np
from scipy import ndimage

_RANK = {6: 1, 18: 2, 26: 3}
_FACES = ndimage.generate_binary_structure(3, 1)


class Filled(NamedTuple):
  volume: np.ndarray      # vol's dtype, shape and memory order
  filled: int             # holes filled
  open: int               # holes with a voxel on a face of the volume
  multi: int              # enclosed holes whose face neighbours carry two labels or more


def fill_holes(vol: np.ndarray, connectivity: int = 6) -> Filled:
  vol = np.asarray(vol)
  out = vol.copy(order="K")
  holes, n = ndimage.label(vol == 0, ndimage.generate_binary_structure(3, _RANK[connectivity]))
  filled = n_open = multi = 0
  for i, box in enumerate(ndimage.find_objects(holes)):
    if any(s.start == 0 or s.stop == dim for s, dim in zip(box, vol.shape)):
      n_open += 1
      continue
    grown = tuple(slice(s.start - 1, s.stop + 1) for s in box)
    mask = holes[grown] == i + 1
    around = np.unique(vol[grown][ndimage.binary_dilation(mask, _FACES) & ~mask])
    if around.size == 1 and around[0] != 0:
      out[grown][mask] = around[0]
      filled += 1
    else:
      multi += 1
  return Filled(out, filled, n_open, multi)
