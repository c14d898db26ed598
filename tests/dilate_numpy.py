"""A numpy restatement of crackle_amd.dilate, computed from the INPUT array (never from what the code under test
decodes), in the manner of tests/erode_numpy.py.

The volume is padded by one voxel of 0 on every side (a neighbour outside the volume carries no label), and the 6, 18
or 26 shifted views of the padded volume are stacked.  A voxel whose label is not 0 keeps it.  A voxel with label 0
takes the label other than 0 that occurs most often among its views, the smallest of those tied for most often (labels
compared as unsigned integers), or stays 0 when every view shows 0.
"""
import numpy as np

from erode_numpy import offsets


def neighbour_stack(vol: np.ndarray, connectivity: int) -> np.ndarray:
  """[n_offsets, sx, sy, sz]: the labels of every voxel's counted neighbours, 0 outside the volume."""
  vol = np.asarray(vol)
  padded = np.pad(vol, 1, mode="constant", constant_values=0)
  sx, sy, sz = vol.shape
  return np.stack([padded[1 + dx:1 + dx + sx, 1 + dy:1 + dy + sy, 1 + dz:1 + dz + sz] for dx, dy, dz in offsets(connectivity)])


def modes(stack: np.ndarray):
  """(mode, its count) along axis 0 over the entries other than 0, ties to the smallest label; (0, 0) without any."""
  s = np.sort(stack, axis=0)
  best = np.zeros(stack.shape[1:], stack.dtype)
  best_n = np.zeros(stack.shape[1:], np.int64)
  # ascending by label, so that of equal counts the first (smallest) stays
  for i in range(s.shape[0]):
    n = (s == s[i]).sum(axis=0)
    better = (s[i] != 0) & (n > best_n)
    best = np.where(better, s[i], best)
    best_n = np.where(better, n, best_n)
  return best, best_n


def dilate(vol: np.ndarray, connectivity: int = 26) -> np.ndarray:
  """The dilated volume in vol's dtype, shape and memory order."""
  vol = np.asarray(vol)
  if vol.size == 0:
    return vol.copy(order="K")
  best, _ = modes(neighbour_stack(vol, connectivity))
  out = np.where(vol != 0, vol, best).astype(vol.dtype)
  return np.asfortranarray(out) if vol.flags.f_contiguous and not vol.flags.c_contiguous else np.ascontiguousarray(out)
