"""Volumes for crackle_amd.dust, shared by the CPU test that pins what they are (tests/test_dust_cpu.py) and the
GPU tests that run the kernels on them (tests/test_gpu_dust.py).  Plain numpy on top of crackle_amd.synth."""
import numpy as np

from crackle_amd import synth


def voronoi(shape, order="F", dtype=np.uint32, seed=31, cell=(12, 12, 3), modulus=40):
  """Compact cells whose labels recur in separate places (modulus)."""
  lab = synth.as_numpy_f(synth.voronoi_labels(shape, dtype, seed=seed, cell=cell, modulus=modulus))
  return np.ascontiguousarray(lab) if order == "C" else lab


def noise(shape, high, dtype=np.uint8, seed=21):
  return synth.random_labels(shape, dtype, seed=seed, high=high)


def checkerboard(shape=(130, 70, 2)):
  """Labels 1 and 2 alternating along every axis, no zero: at connectivity 6 every voxel is a component of its
  own, at 18 and 26 there are two components of half the voxels each."""
  x, y, z = np.meshgrid(*(np.arange(s) for s in shape), indexing="ij")
  return np.asfortranarray(((x + y + z) % 2 + 1).astype(np.uint8))


def staircase():
  """The one-voxel-thick staircase through (8, 8, 40) of the connected-components tests: one component of 79
  voxels at every connectivity, a chain of 40 unions."""
  lab = np.zeros((8, 8, 40), np.uint8, order="F")
  def at(i):
    return (i % 8 if (i // 8) % 2 == 0 else 7 - i % 8), i // 8
  for z in range(40):
    lab[at(z) + (z,)] = 3
    if z + 1 < 40:
      lab[at(z + 1) + (z,)] = 3
  return lab


def combs():
  """The two interleaved combs of the connected-components tests, joined in the last slice only, and some specks
  of another label in between."""
  lab = np.zeros((33, 12, 10), np.uint16, order="F")
  lab[0:33:4, 1:6, :] = 5
  lab[2:33:4, 6:11, :] = 5
  lab[:, 1, 9] = 5
  lab[:, 10, 9] = 5
  lab[16, :, 9] = 5
  lab[1:33:4, 3, 2] = 8
  return lab


def corner_pieces():
  """Pieces of one label that touch at edges and corners only: 5 components at 6, 3 at 18, 2 at 26."""
  lab = np.zeros((6, 6, 3), np.uint32, order="F")
  lab[0:2, 0:2, 0] = 9
  lab[2:4, 2:4, 0] = 9      # in-plane corner of the first block: an edge neighbour in 3D
  lab[4:6, 4:6, 1] = 9      # corner neighbour of the second block across z
  lab[0, 5, 2] = 9
  lab[0, 4, 1] = 9          # edge neighbour across z
  return lab


def small_on_big():
  """A piece of 3 voxels of label 7 lying against a piece of 48 voxels of label 4, and a speck of label 7 apart."""
  lab = np.zeros((10, 8, 3), np.uint16, order="F")
  lab[1:5, 1:5, 0:3] = 4
  lab[5, 1:4, 1] = 7
  lab[8, 6, 2] = 7
  return lab


def three_and_four():
  """A 3-voxel and a 4-voxel piece of one label."""
  lab = np.zeros((7, 5, 2), np.uint8, order="F")
  lab[0:3, 0, 0] = 6
  lab[4:6, 3:5, 1] = 6
  return lab


def width_stripes(shape, n_labels, n_specks):
  """n_labels distinct labels and no zero: n_labels - n_specks stripes two voxels wide (blocks of 2 x h voxels in
  raster order, labels 1 .. ; the blocks past the last label belong to the last stripe, which stays one piece) and
  n_specks single voxels with labels of their own, each in a corner of a block.  Dusting at threshold 2 removes the
  specks alone."""
  sx, sy, sz = shape
  assert sz == 1 and sx % 2 == 0
  n_stripes = n_labels - n_specks
  h = max(k for k in range(2, sy + 1) if sy % k == 0 and (sx // 2) * (sy // k) >= n_stripes)      # the tallest blocks that give enough of them
  x, y = np.meshgrid(np.arange(sx), np.arange(sy), indexing="ij")
  block = (x // 2) + (sx // 2) * (y // h)
  lab = (np.minimum(block, n_stripes - 1) + 1).astype(np.uint32)
  for i in range(n_specks):
    b = 3 + 5 * i      # the speck takes the first corner of block b
    lab[2 * (b % (sx // 2)), h * (b // (sx // 2))] = n_stripes + 1 + i
  return np.asfortranarray(lab[:, :, None])


def width_stripes_dusted(shape, n_labels, n_specks):
  """width_stripes(...) dusted at threshold 2, connectivity 6: the specks (the highest labels) are gone."""
  vol = width_stripes(shape, n_labels, n_specks)
  return np.asfortranarray(np.where(vol > n_labels - n_specks, 0, vol).astype(vol.dtype))


# (shape, labels in the input, specks, unique values after dust at threshold 2): key widths on both sides of 1 -> 2 and
# 2 -> 4 bytes; byte_width(255) = 1, byte_width(256) = 2, byte_width(65535) = 2, byte_width(65536) = 4
WIDTH_EDGES = [
  ((64, 32, 1), 256, 1, 256),          # 255 + {0}: stays at 2-byte keys
  ((64, 32, 1), 255, 1, 255),          # 254 + {0}: stays at 1-byte keys
  ((64, 32, 1), 256, 2, 255),          # 254 + {0}: drops from 2 to 1 byte
  ((512, 512, 1), 65536, 1, 65536),    # stays at 4-byte keys
  ((512, 512, 1), 65535, 1, 65535),    # stays at 2-byte keys
  ((512, 512, 1), 65536, 2, 65535),    # drops from 4 to 2 bytes
]


def stored_width_drop():
  """The only label above 255 is a speck."""
  lab = np.full((9, 7, 2), 3, np.uint16, order="F")
  lab[0:4, :, 1] = 200
  lab[6, 3, 0] = 300
  return lab


# (id, volume maker, threshold, connectivity, binary_image): every volume the GPU tests dust with a threshold of their own
# choosing; tests/test_dust_cpu.py asserts that each has removed and kept components under the restatement
GPU_CASES = [
  ("voronoi-128x64x9-t50", lambda: voronoi((128, 64, 9)), 50, 26, False),
  ("voronoi-128x64x9-t200", lambda: voronoi((128, 64, 9)), 200, 6, False),
  ("voronoi-97x61x7-t50", lambda: voronoi((97, 61, 7)), 50, 18, False),
  ("voronoi-97x61x7-t200", lambda: voronoi((97, 61, 7)), 200, 26, False),
  ("voronoi-96x80x6-C-t50", lambda: voronoi((96, 80, 6), "C"), 50, 26, False),
  ("voronoi-96x80x6-C-t200", lambda: voronoi((96, 80, 6), "C"), 200, 6, False),
  ("noise-64x48x5-t2", lambda: noise((64, 48, 5), 3), 2, 6, False),
  ("noise-64x48x5-t4", lambda: noise((64, 48, 5), 3), 4, 26, False),
  ("noise-64x48x5-t2-binary", lambda: noise((64, 48, 5), 3), 2, 6, True),
  ("noise-64x48x5-t4-binary", lambda: noise((64, 48, 5), 3), 4, 6, True),
  ("noise-130x70x4-t3", lambda: noise((130, 70, 4), 2), 3, 6, False),
  ("combs-t4", combs, 4, 26, False),
  ("corner-pieces-t3", corner_pieces, 3, 6, False),
  ("small-on-big-t4", small_on_big, 4, 26, False),
  ("medium-256x256x32-t4000", lambda: voronoi((256, 256, 32), seed=5, cell=(32, 32, 8), modulus=50), 4000, 26, False),
]
