"""What crackle_amd.overlay and crackle_amd.mask_by compute, restated in numpy from the two input arrays: the three rules
with their dtype and memory-order rules, and the count of x-runs that the profile line reports.  Pinned by a literal
triple loop in tests/test_combine_cpu.py."""
import numpy as np

RULES = ("overlay", "keep", "drop")      # overlay(a, b), mask_by(a, b), mask_by(a, b, invert=True)


def out_dtype(a_dtype, b_dtype, rule):
  """overlay: the unsigned dtype of the larger of the two widths; mask_by: a's."""
  if rule != "overlay":
    return np.dtype(a_dtype)
  return np.dtype("u%d" % max(np.dtype(a_dtype).itemsize, np.dtype(b_dtype).itemsize))


def like(a, out):
  """out in a's memory order (a volume that is both, a single column say, counts as Fortran order)."""
  return np.ascontiguousarray(out) if (a.flags.c_contiguous and not a.flags.f_contiguous) else np.asfortranarray(out)


def combine(a, b, rule):
  assert a.shape == b.shape and rule in RULES
  dt = out_dtype(a.dtype, b.dtype, rule)
  wide_a, there = a.astype(dt), b != 0
  if rule == "overlay":
    out = np.where(there, b.astype(dt), wide_a)
  elif rule == "keep":
    out = np.where(there, wide_a, dt.type(0))
  else:
    out = np.where(there, dt.type(0), wide_a)
  return like(a, out.astype(dt))


def overlay(a, b):
  return combine(a, b, "overlay")


def mask_by(a, b, invert=False):
  return combine(a, b, "drop" if invert else "keep")


def x_runs(vol):
  """Runs of equal labels along x: one per row and one more per change."""
  v = np.asarray(vol)
  return int((v[1:] != v[:-1]).sum()) + v.shape[1] * v.shape[2]


def predicted_counts(table, rule):
  """{label: voxels} of the combined volume from the contingency table {(a, b): voxels} of the two inputs."""
  out = {}
  for (a, b), n in table.items():
    label = (b if b else a) if rule == "overlay" else ((a if b else 0) if rule == "keep" else (0 if b else a))
    out[label] = out.get(label, 0) + n
  return out
