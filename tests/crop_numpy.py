"""What crackle_amd.crop computes, restated in numpy from the input array: the contiguous copy of the box in the volume's
own memory order; the count of x-runs that the profile line reports; and the grid of chunk boxes, restated independently
of the package's chunk_boxes.  Pinned by literal loops in tests/test_crop_cpu.py."""
import numpy as np


def like(a, out):
  """out in a's memory order (a volume that is both, a single column say, counts as Fortran order)."""
  return np.ascontiguousarray(out) if (a.flags.c_contiguous and not a.flags.f_contiguous) else np.asfortranarray(out)


def crop(vol, box):
  """box: (x0, x1, y0, y1, z0, z1).  A copy, never a view: the box owns its memory, as the decoded stream does."""
  x0, x1, y0, y1, z0, z1 = box
  return like(vol, np.array(vol[x0:x1, y0:y1, z0:z1]))


def slices(box):
  """The box as the index expression that crop() and cutout() take."""
  x0, x1, y0, y1, z0, z1 = box
  return (slice(x0, x1), slice(y0, y1), slice(z0, z1))


def in_bounds(box, shape):
  return all(0 <= box[2 * k] <= box[2 * k + 1] <= shape[k] for k in range(3))


def x_runs(vol):
  """Runs of equal labels along x: one per row and one more per change."""
  v = np.asarray(vol)
  return int((v[1:] != v[:-1]).sum()) + v.shape[1] * v.shape[2]


def chunk_boxes(shape, chunk_size):
  """The grid that tiles `shape` from (0, 0, 0) with chunks of `chunk_size`, x fastest, counted by chunk index (the
  package's walks the origins)."""
  nx, ny, nz = (-(-s // c) for s, c in zip(shape, chunk_size))
  out = []
  for k in range(nz):
    for j in range(ny):
      for i in range(nx):
        lo = (i * chunk_size[0], j * chunk_size[1], k * chunk_size[2])
        hi = tuple(min(l + c, s) for l, c, s in zip(lo, chunk_size, shape))
        out.append((lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]))
  return out
