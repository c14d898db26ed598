"""Volumes, slab depths and the case table for the sharded codec on uneven slabs and at the thresholds of its label
merge (crackle_amd/distributed.py).  Plain numpy, no GPU; shared by tests/test_sharded_slabs_cpu.py, which pins every
volume to the counts claimed here and runs the table on the CPU oracle, and tests/test_gpu_sharded_slabs.py, which
runs it with four HIP ranks.

A case is (volume, depths, markov order, pins, env): rank r of four holds depths[r] consecutive slices behind those of
the ranks before it, possibly none.  CLAIMS states what each volume is there for, per slab of the depths it names:
the distinct labels of every slab and of the whole volume, the slabs without a crack edge, and the equal linear
neighbours (pixel_pairs) against voxels // 2."""
import functools

import numpy as np

import threshold_volumes

WORLD = 4

# ---- depths (world 4; the sum is the volume's sz) -------------------------------------------------------------------
UNEQUAL = (3, 3, 2, 2)
ONE_SLICE_ENDS = (1, 7, 1, 1)
EMPTY_MIDDLE = (4, 0, 5, 1)        # an empty rank between two slabs
EMPTY_ENDS = (0, 6, 4, 0)          # rank 0 empty (the stream's header, model and unique list are not its own), last rank empty
ONE_SLAB = (0, 0, 10, 0)           # one slab, not on rank 0
PAIR_OVER_EMPTY = (2, 0, 2, 0)     # pairs_*: the deciding pair straddles an empty rank
TWO_ONES = (1, 1, 0, 0)            # two_slices: pins are allowed (two slices) although every slab has one
ONE_ONE = (1, 0, 0, 0)             # slice0: pins asked, not used
ALL_ONES = (1, 1, 1, 1)            # merge volumes

MERGE_SHAPE = (260, 256, 4)
PAIRS_H = 64 * 33 * 4 // 2


def _voronoi10(dtype=np.uint32, offset=0):
  from crackle_amd import synth
  return synth.as_numpy_f(synth.voronoi_labels((96, 80, 10), dtype, seed=51, cell=(16, 16, 4), offset=offset)).copy(order="F")


def _u64_10():
  v = _voronoi10(np.uint64, offset=1 << 40)
  v[5:11, 7:12, 0] = (1 << 63) + 5
  v[40:52, 30:33, 9] = (1 << 64) - 1
  return v


def _flat_ends():
  v = _voronoi10()
  for z in (0, 1, 2, 8, 9):
    v[:, :, z] = 5000 + z
  return v


def merge_slice(n, base, dtype=np.uint32):
  """One slice of MERGE_SHAPE with the n labels base .. base + n - 1 as runs in raster order."""
  sx, sy, _ = MERGE_SHAPE
  return (np.arange(sx * sy, dtype=np.int64) * n // (sx * sy) + base).reshape(sy, sx).T.astype(dtype)


def merge(n, shared, dtype=np.uint32, n1=None):
  """Slices 0 and 1 hold the labels 1 .. n, slices 2 and 3 the n1 (default n) labels from 1 + n - shared on: every
  one-slice slab has n (n1) distinct labels, the whole volume n + n1 - shared."""
  n1 = n if n1 is None else n1
  lo, hi = merge_slice(n, 1, dtype), merge_slice(n1, 1 + n - shared, dtype)
  return np.asfortranarray(np.stack([lo, lo, hi, hi], axis=2))


def _lone_label():
  """Slice 0 is one label (one component: N = 1) beside 70 000 labels in the other three slices; its own label is in
  none of them."""
  parts = [np.full(MERGE_SHAPE[:2], 123456, np.uint32)] + [merge_slice(30000, base) for base in (1, 20001, 40001)]
  return np.asfortranarray(np.stack(parts, axis=2))


_BUILDERS = {
  "voronoi10": _voronoi10,
  "u64_10": _u64_10,
  "flat_ends": _flat_ends,
  "pairs_at_half": lambda: threshold_volumes.sharded_volume(PAIRS_H),
  "pairs_below_half": lambda: threshold_volumes.sharded_volume(PAIRS_H - 1),
  "two_slices": lambda: _voronoi10()[:, :, :2],
  "slice0": lambda: _voronoi10()[:, :, :1],
  "merge200_255": lambda: merge(200, 145, np.uint16),
  "merge200_256": lambda: merge(200, 144, np.uint16),
  "merge200_257": lambda: merge(200, 143, np.uint16),
  "merge40000_65535": lambda: merge(40000, 14465),
  "merge40000_65536": lambda: merge(40000, 14464),
  "merge40000_65537": lambda: merge(40000, 14463),
  "merge255_1": lambda: merge(255, 0, np.uint16, n1=1),
  "lone_label": _lone_label,
}
MERGE_VOLUMES = tuple(k for k in _BUILDERS if k.startswith("merge")) + ("lone_label",)


@functools.lru_cache(maxsize=None)
def volume(name):
  """The F-ordered (sx, sy, sz) volume of that name, built once per process and read-only."""
  v = np.asfortranarray(_BUILDERS[name]())
  v.setflags(write=False)
  return v


def bounds(depths):
  """[(z0, z1)] of every rank."""
  out, z = [], 0
  for d in depths:
    out.append((z, z + d))
    z += d
  return out


def slab(vol, depths, rank):
  z0, z1 = bounds(depths)[rank]
  return np.asfortranarray(vol[:, :, z0:z1])


def crack_edges(arr):
  """Voxel faces inside the slices of `arr` that separate two labels."""
  return int(np.count_nonzero(arr[1:] != arr[:-1]) + np.count_nonzero(arr[:, 1:] != arr[:, :-1]))


def measure(name, depths):
  """What CLAIMS states, counted: (labels per slab, labels of the whole volume, ranks whose slab has slices but no
  crack edge, pixel_pairs, voxels // 2)."""
  vol = volume(name)
  per, crackless = [], []
  for r in range(len(depths)):
    s = slab(vol, depths, r)
    per.append(int(np.unique(s).size))
    if s.size and crack_edges(s) == 0:
      crackless.append(r)
  return tuple(per), int(np.unique(vol).size), tuple(crackless), threshold_volumes.pairs(vol), vol.size // 2


# name -> (depths, labels per slab, labels merged, slabs without a crack edge, pixel_pairs, voxels // 2)
CLAIMS = {
  "voronoi10": (UNEQUAL, (80, 86, 67, 69), 163, (), 69215, 38400),
  "u64_10": (ONE_SLICE_ENDS, (62, 124, 58, 59), 165, (), 69208, 38400),
  "flat_ends": (UNEQUAL, (3, 86, 67, 2), 110, (0, 3), 72969, 38400),
  "pairs_at_half": (PAIR_OVER_EMPTY, (3, 0, 1, 0), 3, (2,), PAIRS_H, PAIRS_H),
  "pairs_below_half": (PAIR_OVER_EMPTY, (2, 0, 1, 0), 3, (2,), PAIRS_H - 1, PAIRS_H),
  "two_slices": (TWO_ONES, (61, 56, 0, 0), 71, (), 13864, 7680),
  "slice0": (ONE_ONE, (61, 0, 0, 0), 61, (), 6906, 3840),
  "merge200_255": (ALL_ONES, (200, 200, 200, 200), 255, (), 265440, 133120),
  "merge200_256": (ALL_ONES, (200, 200, 200, 200), 256, (), 265440, 133120),
  "merge200_257": (ALL_ONES, (200, 200, 200, 200), 257, (), 265440, 133120),
  "merge40000_65535": (ALL_ONES, (40000, 40000, 40000, 40000), 65535, (), 106240, 133120),
  "merge40000_65536": (ALL_ONES, (40000, 40000, 40000, 40000), 65536, (), 106240, 133120),
  "merge40000_65537": (ALL_ONES, (40000, 40000, 40000, 40000), 65537, (), 106240, 133120),
  "merge255_1": (ALL_ONES, (255, 255, 1, 1), 256, (2, 3), 265729, 133120),
  "lone_label": (ALL_ONES, (1, 30000, 30000, 30000), 70001, (0,), 176239, 133120),
}

# crack format the header must show (tests/test_gpu_sharded.py asserts the same of its two-rank cases)
CRACK_FORMAT = {"pairs_at_half": 0, "pairs_below_half": 1}

ENVS = ("CKL_SHARDED_LEGACY", "CKL_TEST_MERGE_FAIL", "CKL_TEST_NO_COLLECT", "CKL_PINS_ON_ROOT")

# (volume, depths, markov order, pins, env)
CASES = [
  # every depth tuple, flat, order 0
  ("voronoi10", UNEQUAL, 0, False, None), ("voronoi10", ONE_SLICE_ENDS, 0, False, None), ("voronoi10", EMPTY_MIDDLE, 0, False, None),
  ("voronoi10", EMPTY_ENDS, 0, False, None), ("voronoi10", ONE_SLAB, 0, False, None),
  ("pairs_at_half", PAIR_OVER_EMPTY, 0, False, None), ("pairs_below_half", PAIR_OVER_EMPTY, 0, False, None),
  ("two_slices", TWO_ONES, 0, False, None), ("slice0", ONE_ONE, 0, False, None),
  # pins decided by the whole volume's depth, not the slab's
  ("two_slices", TWO_ONES, 0, True, None), ("slice0", ONE_ONE, 0, True, None),
  # unequal, one-slice and empty-in-the-middle depths through every road of the label merge and the pin stage
  ("voronoi10", UNEQUAL, 3, True, "CKL_TEST_NO_COLLECT"), ("voronoi10", ONE_SLICE_ENDS, 3, True, "CKL_TEST_NO_COLLECT"), ("voronoi10", EMPTY_MIDDLE, 3, True, "CKL_TEST_NO_COLLECT"),
  ("voronoi10", UNEQUAL, 0, True, "CKL_PINS_ON_ROOT"), ("voronoi10", ONE_SLICE_ENDS, 0, True, "CKL_PINS_ON_ROOT"), ("voronoi10", EMPTY_MIDDLE, 0, True, "CKL_PINS_ON_ROOT"),
  ("voronoi10", UNEQUAL, 0, False, "CKL_SHARDED_LEGACY"), ("voronoi10", ONE_SLICE_ENDS, 0, False, "CKL_SHARDED_LEGACY"), ("voronoi10", EMPTY_MIDDLE, 0, False, "CKL_SHARDED_LEGACY"),
  ("voronoi10", UNEQUAL, 0, False, "CKL_TEST_MERGE_FAIL"), ("voronoi10", ONE_SLICE_ENDS, 0, False, "CKL_TEST_MERGE_FAIL"), ("voronoi10", EMPTY_MIDDLE, 0, False, "CKL_TEST_MERGE_FAIL"),
  # rank 0 empty: header, model, unique list and pin section come from the first rank that holds slices
  ("voronoi10", EMPTY_ENDS, 3, True, "CKL_TEST_NO_COLLECT"), ("voronoi10", EMPTY_ENDS, 2, True, "CKL_PINS_ON_ROOT"), ("voronoi10", EMPTY_ENDS, 3, False, "CKL_SHARDED_LEGACY"),
  ("voronoi10", ONE_SLAB, 3, True, None),
  # slabs without any crack under a model that the slabs with cracks decide
  ("flat_ends", UNEQUAL, 3, False, None), ("flat_ends", UNEQUAL, 3, True, None),
  # uint64 labels above 2^63 in the one-slice end slabs / beside empty ranks
  ("u64_10", ONE_SLICE_ENDS, 0, False, None), ("u64_10", EMPTY_ENDS, 5, True, None),
]
# the merged unique list is wider than every slab's own: in the encoder's exchange and merged after the encode
CASES += [(name, ALL_ONES, 0, False, env) for name in MERGE_VOLUMES for env in (None, "CKL_SHARDED_LEGACY")]


def case_id(case):
  name, depths, order, pins, env = case
  return f"{name}-{'.'.join(str(d) for d in depths)}-m{order}-{'pins' if pins else 'flat'}{'-' + env if env else ''}"


# ---- four ranks, one spawn for a whole table -------------------------------------------------------------------------
def free_port():
  import socket
  s = socket.socket()
  s.bind(("127.0.0.1", 0))
  p = s.getsockname()[1]
  s.close()
  return p


def run_table(worker, n_cases, timeout):
  """Starts worker(rank, port, queue) on WORLD spawned processes; every rank puts (rank, index, ..., error or None)
  on the queue once per case.  Stops at the first reported error, or when no rank reports for `timeout` seconds: the
  children are ended and nothing is tried again.  Returns ({(rank, index): the rest of the tuple}, why it stopped or
  None)."""
  import multiprocessing
  import queue
  ctx = multiprocessing.get_context("spawn")
  q = ctx.Queue()
  port = free_port()
  procs = [ctx.Process(target=worker, args=(r, port, q)) for r in range(WORLD)]
  for p in procs:
    p.start()
  results, stopped = {}, None
  for _ in range(WORLD * n_cases):
    try:
      got = q.get(timeout=timeout)
    except queue.Empty:
      stopped = f"no rank reported for {timeout} s"
      break
    results[(got[0], got[1])] = got[2:]
    if got[-1]:
      stopped = f"rank {got[0]}, case {got[1]}: {got[-1]}"
      break
  for p in procs:
    if stopped is None:
      p.join(timeout=60)
    if p.is_alive():
      p.terminate()
      p.join(timeout=10)
  if stopped is None and any(p.exitcode != 0 for p in procs):
    stopped = f"exit codes {[p.exitcode for p in procs]}"
  return results, stopped
