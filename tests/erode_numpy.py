"""A numpy restatement of crackle_amd.erode, computed from the INPUT array (never from what the code under test
decodes), in the manner of tests/fill_holes_numpy.py.

The volume is padded by one voxel on every side: with the constant 0 for erode_border (a neighbour outside the volume
is different from every label that could be kept), by edge replication without it (a neighbour outside the volume is
the voxel's own row, column or slice again, so it is ignored).  A voxel keeps its label when the label is not 0 and
each of the 6, 18 or 26 shifted views of the padded volume shows the same value there.
"""
import itertools

import numpy as np


def offsets(connectivity):
  """(dx, dy, dz) in {-1, 0, 1}^3 with 0 < |dx| + |dy| + |dz| <= 1, 2, 3."""
  reach = {6: 1, 18: 2, 26: 3}[connectivity]
  return [o for o in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(map(abs, o)) <= reach]


def erode(vol: np.ndarray, connectivity: int = 26, erode_border: bool = True) -> np.ndarray:
  """The eroded volume in vol's dtype, shape and memory order."""
  vol = np.asarray(vol)
  if vol.size == 0:
    return vol.copy(order="K")
  padded = np.pad(vol, 1, mode="constant", constant_values=0) if erode_border else np.pad(vol, 1, mode="edge")
  sx, sy, sz = vol.shape
  keep = vol != 0
  for dx, dy, dz in offsets(connectivity):
    keep &= padded[1 + dx:1 + dx + sx, 1 + dy:1 + dy + sy, 1 + dz:1 + dz + sz] == vol
  out = np.where(keep, vol, vol.dtype.type(0)).astype(vol.dtype)
  return np.asfortranarray(out) if vol.flags.f_contiguous and not vol.flags.c_contiguous else np.ascontiguousarray(out)
