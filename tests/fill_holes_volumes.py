"""Volumes for crackle_amd.fill_holes, shared by the CPU test that pins what they are (tests/test_fill_holes_cpu.py)
and the GPU tests that run the kernels on them (tests/test_gpu_fill_holes.py).  Plain numpy on top of
crackle_amd.synth and tests/dust_volumes.py."""
import numpy as np

import dust_volumes

SHAPE = (12, 10, 5)      # sx is no multiple of 32; three inner slices
HOLE = (5, 4, 2)         # one voxel away from no face
FACE_STEPS = {           # the six face neighbours of a voxel, by what the scan kernel calls them
  "run-before": (-1, 0, 0), "run-after": (1, 0, 0), "row-above": (0, -1, 0), "row-below": (0, 1, 0),
  "slice-before": (0, 0, -1), "slice-after": (0, 0, 1),
}


def block(shape=SHAPE, label=4, dtype=np.uint16):
  return np.full(shape, label, dtype, order="F")


def one_voxel(at=HOLE):
  """A one-voxel hole in a block of label 4."""
  vol = block()
  vol[at] = 0
  return vol


def at_face(axis, last, inset=0):
  """The one-voxel hole moved onto a face of the volume (inset 0) or one voxel away from it (inset 1)."""
  at = list(HOLE)
  at[axis] = SHAPE[axis] - 1 - inset if last else inset
  return one_voxel(tuple(at))


def second_label_by_face(direction):
  """The one-voxel hole with one voxel of label 9 as its face neighbour in the given direction."""
  vol = one_voxel()
  vol[tuple(h + s for h, s in zip(HOLE, FACE_STEPS[direction]))] = 9
  return vol


def second_label_diagonal():
  """The one-voxel hole with label 9 on edge and corner neighbours only: in the slice, across rows and across slices."""
  vol = one_voxel()
  x, y, z = HOLE
  vol[x - 1, y - 1, z] = 9
  vol[x + 1, y, z + 1] = 9
  vol[x, y + 1, z - 1] = 9
  vol[x + 1, y + 1, z + 1] = 9
  vol[x - 1, y + 1, z - 1] = 9
  return vol


def three_slices():
  """A hole through the three inner slices with a different cross-section in each."""
  vol = block()
  vol[4:7, 4, 1] = 0
  vol[3:8, 3:6, 2] = 0
  vol[5, 4:6, 3] = 0
  return vol


def edge_touching_holes():
  """The one-voxel hole and, across an edge of it, a hole that runs to the face y = sy - 1: at connectivity 6 the
  first fills, at 18 and 26 both are one open hole."""
  vol = one_voxel()
  vol[HOLE[0] + 1, HOLE[1] + 1:, HOLE[2]] = 0
  return vol


def corner_touching_holes():
  """The one-voxel hole and, across a corner of it, a hole that runs to the face z = sz - 1: at connectivity 6 and 18
  the first fills, at 26 both are one open hole."""
  vol = one_voxel()
  vol[HOLE[0] + 1, HOLE[1] + 1, HOLE[2] + 1:] = 0
  return vol


def speck_in_block():
  """A block of label 4 with a speck of label 7: mask(stream, [7]) or dust(stream, 2) turns the speck into a hole."""
  vol = block()
  vol[HOLE] = 7
  return vol


def bar_in_void():
  """A void in a block of label 4 with a bar of label 7 across its middle slice.  Once the bar is label 0 (mask(), or
  dust() at threshold 4) the void's middle slice holds three 2D components of label 0 with false boundaries between
  them: one hole all the same."""
  vol = block()
  vol[4:7, 3:6, 1:4] = 0
  vol[4:7, 4, 2] = 7
  return vol


def punched(shape, order="F", seed=77, boxes=300, cell=(16, 16, 4)):
  """dust_volumes.voronoi (compact cells whose labels recur; a larger cell than the dust tests use, so that more
  voids lie inside one) with random boxes of 1 - 3 voxels a side set to 0: voids inside a cell, voids between cells
  and voids on the faces of the volume."""
  vol = dust_volumes.voronoi(shape, "F", cell=cell).copy(order="F")
  rng = np.random.RandomState(seed)
  for _ in range(boxes):
    side = rng.randint(1, 4, 3)
    at = [rng.randint(0, s - d + 1) for s, d in zip(shape, side)]
    vol[tuple(slice(a, a + d) for a, d in zip(at, side))] = 0
  return np.ascontiguousarray(vol) if order == "C" else vol


PUNCHED = [((128, 64, 9), "F"), ((97, 61, 7), "F"), ((96, 80, 6), "C")]


def pocked(shape=(130, 70, 4)):
  """A block of one label with one-voxel holes at every second position of the two inner slices (odd x and y in slice
  1, even x and y in slice 2, so that no two share a face): thousands of holes with the same enclosing label, and
  more than 2048 runs a slice."""
  vol = np.full(shape, 3, np.uint8, order="F")
  vol[1:-1:2, 1:-1:2, 1] = 0
  vol[2:-1:2, 2:-1:2, 2] = 0
  return vol


def hollow_box(variant="closed", shape=(130, 70, 5)):
  """A box of label 6 whose cavity is ONE hole of thousands of runs: pillars of the box's own label stand at every
  second x of every second row, so a slice of the cavity has more than 4000 runs of label 0, spread over three
  workgroups, in each of three slices.  "closed": fillable.  "second-label": one wall voxel next to the cavity has
  label 9.  "tunnel": one wall voxel next to the cavity is 0, which opens the cavity to the face y = 0."""
  vol = np.full(shape, 6, np.uint16, order="F")
  vol[1:-1, 1:-1, 1:-1] = 0
  vol[2:-2:2, 2:-2:2, 1:-1] = 6
  if variant == "second-label":
    vol[shape[0] // 2 + 1, 0, 2] = 9
  elif variant == "tunnel":
    vol[shape[0] // 2 + 1, 0, 2] = 0
  else:
    assert variant == "closed"
  return vol


def all_holes_fillable(n_labels=256):
  """256 blocks of 4 x 4 x 3 voxels with labels 1 .. n_labels (256, or 255: the last two blocks share a label then),
  each with a one-voxel hole inside: every background voxel is a fillable hole, and label 0 leaves the unique list.
  Keys are one byte wide up to 255 values: 256 labels and 0 are 257 values before and 256 after, 2-byte keys both
  times; 255 labels and 0 are 256 values before and 255 after, and the keys drop from 2 bytes to 1."""
  assert n_labels in (255, 256)
  x, y = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
  lab = np.minimum(1 + x // 4 + 16 * (y // 4), n_labels).astype(np.uint16)
  vol = np.asfortranarray(np.repeat(lab[:, :, None], 3, axis=2))
  vol[1::4, 1::4, 1] = 0
  return vol


def for_dtype(dtype):
  """Two labels, a fillable hole in each, one hole between them and one on a face."""
  vol = np.full((31, 29, 5), 2, dtype, order="F")
  vol[16:, :, :] = 5
  if np.dtype(dtype) == np.uint64:
    vol = np.asfortranarray(vol * np.uint64(1 << 40))
  vol[3:6, 4:7, 1:3] = 0
  vol[20:23, 9, 2:4] = 0
  vol[15:17, 20, 2] = 0
  vol[9, 0:3, 1] = 0
  return vol


# (id, volume maker): the volumes of the GPU tests apart from the hand-written minimal cases
GPU_VOLUMES = [
  ("three-slices", three_slices),
  ("bar-in-void", bar_in_void),
  ("pocked", pocked),
  ("noise-130x70x4", lambda: dust_volumes.noise((130, 70, 4), 2)),
  ("hollow-box", hollow_box),
  ("hollow-box-second-label", lambda: hollow_box("second-label")),
  ("hollow-box-tunnel", lambda: hollow_box("tunnel")),
  ("all-holes-fillable", all_holes_fillable),
] + [("punched-%dx%dx%d-%s" % (shape + (order,)), lambda shape=shape, order=order: punched(shape, order)) for shape, order in PUNCHED]
