"""Volumes and edits for paste() (crackle_amd/array.py; ckl_paste and k_paste_box in crackle_amd/csrc/ckl_paste.hip).
Plain numpy on top of crackle_amd.synth; shared by the CPU test that pins the precondition of every byte claim
(tests/test_paste_cpu.py) and the GPU tests that run the kernels (tests/test_gpu_paste.py).

A splice case is a volume V, an index expression whose z-range is not the whole depth, and the data assigned there.
paste() encodes the edited slab under V's crack format and stacks it between the untouched slices of V's stream; that
is compress(V') byte for byte exactly when compress would pick the same crack format for V' as for V (the format is one
decision over the whole volume, src/crackle.hpp:48-55), which the CPU test asserts with the checker for every case
below."""
import functools

import numpy as np

from crackle_amd import synth

S = np.s_

# the three slice geometries of tests/test_gpu_cutout.py and a uint64 one; 97 and 33 are odd, so no two rows of a box
# start at the same offset modulo 16 bytes.  The last one is a C-order stream whose width is no multiple of 4: ckl_paste
# decodes its slab x fastest (RunRequest::x_fastest), which for such a width is k_paint_runs<OUT, false> in mode 1, a
# kernel that a fortran_order stream of that width reaches without the flag and a 96 wide C-order stream never
GEOMETRIES = [((97, 61, 7), np.uint16, "F"), ((128, 64, 9), np.uint32, "F"), ((96, 80, 6), np.uint8, "C"), ((33, 17, 5), np.uint64, "F"),
              ((90, 61, 5), np.uint32, "C")]
GEOMETRY_IDS = ["97x61x7-u16-F", "128x64x9-u32-F", "96x80x6-u8-C", "33x17x5-u64-F", "90x61x5-u32-C"]


@functools.lru_cache(maxsize=None)
def _voronoi(shape, dtype, order, seed):
  vol = synth.as_numpy_f(synth.voronoi_labels(shape, dtype, seed=seed, cell=(8, 8, 3), offset=(1 << 40) if np.dtype(dtype) == np.uint64 else 0))
  vol = np.ascontiguousarray(vol) if order == "C" else np.asfortranarray(vol)
  vol.setflags(write=False)
  return vol


def volume(shape, dtype, order):
  """The volume the streams are made from (read-only; edits go into a copy)."""
  return _voronoi(shape, np.dtype(dtype).type, order, 31)


def other(shape, dtype, order):
  """Another segmentation of the same shape: where pasted data comes from."""
  return _voronoi(shape, np.dtype(dtype).type, order, 47)


def edited(vol, idx, data):
  """numpy's V[idx] = data on a copy that keeps V's memory order."""
  out = vol.copy(order="K")
  out[idx] = data
  return out


class Splice:
  def __init__(self, id, geometry, idx, fill=None):
    self.id, self.geometry, self.idx, self.fill = id, geometry, idx, fill

  def volume(self):
    return volume(*self.geometry)

  def data(self):
    """The scalar fill, or the same box of the other segmentation."""
    return self.fill if self.fill is not None else other(*self.geometry)[self.idx]

  def edited(self):
    return edited(self.volume(), self.idx, self.data())

  def __repr__(self):
    return self.id


# z0 = 0 (nothing before the slab), z1 = sz (nothing after it), the slices before the last one, and ranges in the middle
SPLICES = [
  Splice("u16-first-slices", GEOMETRIES[0], S[5:50, 3:40, 0:2]),
  Splice("u16-last-slice-fill", GEOMETRIES[0], S[10:20, :, 6:7], fill=7),
  Splice("u16-all-but-the-last-slice", GEOMETRIES[0], S[90:, 1:60, 0:6]),
  Splice("u32-middle", GEOMETRIES[1], S[31:97, 1:63, 3:6]),
  Splice("u32-one-slice-whole-plane", GEOMETRIES[1], S[:, :, 4]),
  Splice("u8-C-middle", GEOMETRIES[2], S[:, 10:30, 2:4]),
  Splice("u8-C-first-slice-fill", GEOMETRIES[2], S[3:77, 5:9, 0], fill=201),
  Splice("u64-middle", GEOMETRIES[3], S[1:30, 2:9, 1:4]),
  Splice("u32-C-odd-width-middle", GEOMETRIES[4], S[3:80, 5:50, 1:3]),
  Splice("u32-C-odd-width-last-slices-fill", GEOMETRIES[4], S[:, 7:9, 3:], fill=70000),
]


def smooth_and_noise():
  """(V, idx, data): binary noise over two whole slices of a smooth Voronoi volume.  The slab alone would be encoded
  PERMISSIBLE (noise: fewer than half of its neighbours are equal), the volume is IMPERMISSIBLE before and after."""
  vol = volume(*GEOMETRIES[1])
  idx = S[:, :, 3:5]
  data = synth.random_labels((128, 64, 2), np.uint32, seed=13, high=2)
  return vol, idx, data


def linear_pairs(arr):
  """lib::pixel_pairs (src/lib.hpp:249-256): equal neighbours of the x-fastest sequence."""
  f = np.asarray(arr).reshape(-1, order="F")
  return int(np.count_nonzero(f[1:] == f[:-1]))


def permissible(arr):
  """The crack format compress picks (src/crackle.hpp:48-55)."""
  return linear_pairs(arr) < np.asarray(arr).size // 2
