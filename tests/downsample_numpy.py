"""crackle_amd.downsample restated in plain numpy, from the voxels: what the device computes from the run tables.

(2, 2, 1): the reference's rule (src/operations.hpp:1254-1293).  With a, b, c, d at (x, y), (x + 1, y), (x, y + 1),
(x + 1, y + 1): a == b -> a, a == c -> a, b == c -> b, else d; a block cut by an odd sx or sy copies a.
(2, 2, 2): the label that occurs most often among the block's voxels that exist, ties to the smallest label compared as
unsigned values.  Label 0 is an ordinary label in both.  The output has shape ceil(s / f) per axis, the input's dtype
and its memory order."""
import numpy as np

FACTORS = ((2, 2, 1), (2, 2, 2))


def pooled_shape(shape, factor):
  return tuple(-(-s // f) for s, f in zip(shape, factor))


def block_stack(vol, factor):
  """(stack, exists): [2 * 2 * fz] + the pooled shape each; entry dx + 2 dy + 4 dz is the block's voxel at that offset
  (0 where the volume ends before it), and whether it exists."""
  v = np.asarray(vol)
  assert tuple(factor) in FACTORS and v.ndim == 3
  fz = factor[2]
  sx, sy, sz = v.shape
  ox, oy, oz = pooled_shape(v.shape, factor)
  pad = np.zeros((2 * ox, 2 * oy, fz * oz), v.dtype)
  pad[:sx, :sy, :sz] = v
  ex = np.zeros(pad.shape, bool)
  ex[:sx, :sy, :sz] = True
  at = [(slice(dx, None, 2), slice(dy, None, 2), slice(dz, None, fz)) for dz in range(fz) for dy in range(2) for dx in range(2)]
  return np.stack([pad[s] for s in at]), np.stack([ex[s] for s in at])


def modes(stack, exists):
  """(the most frequent label among the entries that exist, ties to the smallest; how often it occurs)."""
  counts = np.zeros(stack.shape, np.int64)
  for i in range(stack.shape[0]):
    counts[i] = ((stack == stack[i]) & exists).sum(axis=0)
  counts[~exists] = 0
  top = counts.max(axis=0)
  big = np.iinfo(stack.dtype).max
  return np.where(exists & (counts == top), stack, big).min(axis=0), top


def reference_rule(stack, exists):
  a, b, c, d = stack[:4]
  full = exists[3]      # (x + 1, y + 1) exists: the block is not cut
  return np.where(full, np.where((a == b) | (a == c), a, np.where(b == c, b, d)), a)


def _like(vol, out):
  out = out.astype(vol.dtype, copy=False)
  return np.ascontiguousarray(out) if (vol.flags.c_contiguous and not vol.flags.f_contiguous) else np.asfortranarray(out)


def downsample(vol, factor=(2, 2, 1)):
  factor = tuple(factor)
  stack, exists = block_stack(vol, factor)
  out = reference_rule(stack, exists) if factor == (2, 2, 1) else modes(stack, exists)[0]
  return _like(vol, out)


def pyramid(vol, factor, num_mips):
  levels = []
  for _ in range(num_mips):
    vol = downsample(vol, factor)
    levels.append(vol)
  return levels


def pooled_runs(pooled):
  """Runs of equal labels along x in the pooled volume: one per row and one more per change."""
  p = np.asarray(pooled)
  return int((p[1:] != p[:-1]).sum()) + p.shape[1] * p.shape[2]


def stats(vol, factor):
  """Shares of the output voxels (issue tables)."""
  factor = tuple(factor)
  stack, exists = block_stack(vol, factor)
  n = max(1, exists[0].size)
  first = stack[0]
  uniform = ((stack == first) | ~exists).all(axis=0)
  mode, top = modes(stack, exists)
  if factor == (2, 2, 1):
    out = reference_rule(stack, exists)
    s = np.sort(stack, axis=0)
    all_differ = exists.all(axis=0) & (s[1:] != s[:-1]).all(axis=0)
    return dict(not_uniform=float((~uniform).sum()) / n, not_first=float((out != first).sum()) / n,
                not_mode=float((out != mode).sum()) / n, all_differ=float(all_differ.sum()) / n)
  at_top = np.zeros(top.shape, np.int64)      # distinct labels at the top count: every such label is counted `top` times
  for i in range(stack.shape[0]):
    at_top += exists[i] & (((stack == stack[i]) & exists).sum(axis=0) == top)
  big = np.iinfo(stack.dtype).max
  smallest = np.where(exists, stack, big).min(axis=0)
  largest = np.where(exists, stack, 0).max(axis=0)
  return dict(not_uniform=float((~uniform).sum()) / n, tied=float((at_top > top).sum()) / n,
              not_smallest=float((mode != smallest).sum()) / n, not_largest=float((mode != largest).sum()) / n)
