"""GPU tests of the operations that consume a decoded stream without painting it, on both sides of their own size
limits: point_cloud, the label statistics, voxel_connectivity_graph, reencode, mode_pooling_2x2x1, array_equal and
check.  They never take the strip path (decoder_run: `strips = paint && ...`): they run the general pipeline and
then kernels of their own, which choose variants by slice size.

Every threshold is restated here from the host code and computed from the device's properties; the straddle test
asserts that the chosen shapes fall on both of its sides.  Each case compares the device with the checker (the
compiled reference where it was built) and, where a numpy answer is exact, with numpy.  Which side of a threshold
ran is not reported by these operations: the cases rely on the restated predicate, and say so.

Shapes are natural: a CKL_* switch only appears where it is named in the case, with the reason."""
import ctypes as C

import numpy as np
import pytest
import torch

import crackle_amd
from crackle_amd import operations, synth
from crackle_amd import distributed as ckd

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TORCH_DT = {1: torch.uint8, 2: torch.uint16, 4: torch.uint32, 8: torch.uint64}
DTYPES = [np.uint8, np.uint16, np.uint32, np.uint64]
U32 = 0xFFFFFFFF


def _max_lds():
  p = torch.cuda.get_device_properties(0)
  return int(getattr(p, "shared_memory_per_block", 0) or 160 * 1024)


def _max_grid():
  """hipDeviceProp_t::maxGridSize, read through hipDeviceGetAttribute (hipDeviceAttributeMaxGridDimX/Y/Z: entries
  29-31 of hipDeviceAttribute_t in hip_runtime_api.h)."""
  torch.cuda.init()
  hip = C.CDLL("libamdhip64.so")
  out = []
  for attr in (29, 30, 31):
    v = C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(v), attr, 0) == 0
    out.append(v.value)
  return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------
# restated host rules (ckl_operations.hip: decoder_point_cloud, decoder_label_stats)
def pc_lds_visited(sx, sy):
  """The tracer keeps its visited bits in LDS (else in HBM)."""
  return -(-sx * sy // 32) * 4 + 256 <= _max_lds()


def pc_raw_worst(sx, sy):
  """The most contour nodes of one slice: 2 E + sx sy, E = 2 sx sy - sx - sy edges of the pixel grid."""
  return 5 * sx * sy - 2 * sx - 2 * sy


def pc_admitted(sx, sy):
  return pc_raw_worst(sx, sy) <= U32


def pc_first_caps(sx, sy):
  """(raw_cap0, tab_cap0): the first pass's nodes and contours per slice."""
  sxy = sx * sy
  return min(sxy // 2 + 4096, pc_raw_worst(sx, sy)), min(sxy // 32 + 1024, sxy + 1)


def pc_slices_per_chunk(sx, sy):
  """nz: slices per z-chunk of the first pass under the 3 GiB scratch budget."""
  sxy = sx * sy
  raw_cap, tab_cap = pc_first_caps(sx, sy)
  vis_words = (sxy + 31) // 32
  cand_words = ((vis_words + 1) & ~1) + 2 * 64
  per_slice = ((sxy + 3) & ~3) + 4 * vis_words + 8 * cand_words + 4 * raw_cap + 16 * tab_cap + 4 * tab_cap \
      + (0 if pc_lds_visited(sx, sy) else 4 * vis_words) + 16
  return max(1, (3 << 30) // per_slice)


def stats_fit():
  """Per-component accumulators of k_run_stats that fit a workgroup's LDS (36 bytes each, 1 KiB kept back)."""
  return ((_max_lds() - 1024) // 36) & ~1


def stats_lds_comps(max_comp):
  return min((max_comp + 1) & ~1, stats_fit())


def _crack_lds_bytes(n):
  return (n + 2) * 8 + n * 8 + n * 8 + n * 4 + (n // 7 + 48) * 2 + n + 16


def _hbm_row_words():
  """The fewest plane words per row for which k_decode_cracks rasterises into zeroed planes in HBM (decoder_new;
  restated as in tests/test_gpu_shape_edges.py)."""
  budget = max(_max_lds() - 4096, 0)
  n = 5120
  while n > 64 and _crack_lds_bytes(n) > budget:
    n -= 64
  if _crack_lds_bytes(n) > budget:
    n = 0
  n = min(n, 32000)
  lds = max(_crack_lds_bytes(n), budget & ~15)
  return (lds - (n + 2) * 8) // 8 + 1


# ---------------------------------------------------------------------------------------------------------------------
# helpers
def _same_cloud(got, want, what):
  assert sorted(got) == sorted(want), what
  for k in want:
    assert np.array_equal(np.asarray(got[k]).ravel(), np.asarray(want[k]).ravel()), (what, k)


def _voronoi(shape, dt, cell, seed):
  return synth.as_numpy_f(synth.voronoi_labels(shape, dt, seed=seed, cell=cell, device=DEV))


def _exact_stats(arr):
  """{label: (count, centroid, [xmin, ymin, zmin, xmax, ymax, zmax])}: int64 coordinate sums divided once in float64."""
  sx, sy, sz = arr.shape
  flat = arr.reshape(-1, order="F")
  u, inv = np.unique(flat, return_inverse=True)
  inv = inv.reshape(-1)
  idx = np.arange(flat.size, dtype=np.int64)
  coords = (idx % sx, (idx // sx) % sy, idx // (sx * sy))
  cnt = np.bincount(inv, minlength=len(u)).astype(np.int64)
  sums = []
  for c in coords:
    s = np.zeros(len(u), np.int64)
    np.add.at(s, inv, c)
    sums.append(s)
  mins = [np.full(len(u), np.iinfo(np.int64).max), np.full(len(u), np.iinfo(np.int64).max), np.full(len(u), np.iinfo(np.int64).max)]
  maxs = [np.full(len(u), -1, np.int64) for _ in range(3)]
  for k, c in enumerate(coords):
    np.minimum.at(mins[k], inv, c)
    np.maximum.at(maxs[k], inv, c)
  out = {}
  for i, lab in enumerate(u.tolist()):
    cent = np.array([np.float64(s[i]) / np.float64(cnt[i]) for s in sums])
    out[int(lab)] = (int(cnt[i]), cent, [int(m[i]) for m in mins] + [int(m[i]) for m in maxs])
  return out


def _box_quirk(binary, boxes):
  """The reference seeds its boxes from the unique list only (operations.hpp:561-567): a pin stream's background
  colour outside that list has its three minima at 0 (as _reference_box_quirk in tests/test_gpu_parity.py)."""
  h = crackle_amd.header(binary)
  if h.label_format == crackle_amd.LabelFormat.FLAT:
    return boxes
  sz, sw = h.sz, h.stored_data_width
  lb = binary[29 + 4 * (sz + 1):]
  bg = int.from_bytes(lb[:sw], "little")
  n = int.from_bytes(lb[sw:sw + 8], "little")
  uniq = {int.from_bytes(lb[sw + 8 + i * sw: sw + 8 + (i + 1) * sw], "little") for i in range(n)}
  if bg not in uniq and bg in boxes:
    boxes = dict(boxes)
    boxes[bg] = [0, 0, 0] + list(boxes[bg][3:])
  return boxes


def check_stats(binary, arr, checker, what=""):
  """Counts and boxes exact; centroids the float64 division of exact integer sums (array_equal, not allclose)."""
  want = _exact_stats(arr)
  assert crackle_amd.voxel_counts(binary) == {k: v[0] for k, v in want.items()}, what
  assert crackle_amd.voxel_counts(binary) == checker.voxel_counts(binary), what
  cents = crackle_amd.centroids(binary)
  ref_c = checker.centroids(binary)
  assert sorted(cents) == sorted(want) == sorted(ref_c), what
  for k, (_, c, _) in want.items():
    assert cents[k].dtype == np.float64 and np.array_equal(cents[k], c), (what, k, cents[k], c)
    assert np.array_equal(cents[k], ref_c[k]), (what, k)
  boxes = {k: [int(v) for v in b] for k, b in crackle_amd.bounding_boxes(binary, no_slice_conversion=True).items()}
  assert boxes == _box_quirk(binary, {k: v[2] for k, v in want.items()}), what
  assert boxes == {k: [int(v) for v in b] for k, b in checker.bounding_boxes(binary).items()}, what


# ---------------------------------------------------------------------------------------------------------------------
# the shapes of each threshold
PC_VIS = [(1143, 1144), (1144, 1144)]                  # visited bits in LDS / in HBM (160 KiB: between the two)
PC_CHUNK_SLICE = (4096, 4096)
PC_BIG = (16384, 32768)                                # 2^29 pixels
PC_LIMIT = [(26215, 32768), (26216, 32768)]            # the last admitted and the first refused width at this height
STATS_MAX_ODD = 101


def test_consumer_shapes_straddle_every_threshold():
  """Each restated threshold has a case on both of its sides (and the grid limit the deep volumes pass is stated)."""
  sides = {
    "point cloud visited bits in LDS": {pc_lds_visited(*s) for s in PC_VIS},
    "point cloud admitted": {pc_admitted(*s) for s in PC_LIMIT + [PC_BIG]},
    "stats slice in LDS": {n <= stats_lds_comps(stats_fit() + 1) for n in (stats_fit() - 1, stats_fit(), stats_fit() + 1)},
  }
  for name, s in sides.items():
    assert len(s) == 2, (name, s)
  assert pc_admitted(*PC_BIG) and pc_raw_worst(*PC_BIG) >= 1 << 31      # 8 sx sy + 16 wrapped to 16 here
  assert (8 * PC_BIG[0] * PC_BIG[1] + 16) & U32 == 16
  # point cloud first pass: contours and nodes beyond its capacities (asserted from the oracle in the cases)
  raw0, tab0 = pc_first_caps(64, 64)
  assert 64 * 64 > tab0 and (raw0, tab0) == (64 * 64 // 2 + 4096, 64 * 64 // 32 + 1024)
  # z-chunks: nz and nz + 1 slices
  nz = pc_slices_per_chunk(*PC_CHUNK_SLICE)
  assert 2 <= nz < 64 and pc_slices_per_chunk(*PC_CHUNK_SLICE) * 2 > nz + 3
  # stats rounding: an odd max_comp rounds its LDS capacity up
  assert stats_lds_comps(STATS_MAX_ODD) == STATS_MAX_ODD + 1
  # deep volumes: more slices than 2^16
  assert max(DEEP) > 65536 and min(DEEP) == 65535


# ---------------------------------------------------------------------------------------------------------------------
# point cloud
@pytest.mark.parametrize("sx,sy", PC_VIS, ids=[f"{a}x{b}" for a, b in PC_VIS])
def test_point_cloud_visited_bits_lds_or_hbm(sx, sy, checker):
  """Which buffer held the visited bits is not observable: the shapes sit on either side of the restated rule."""
  arr = _voronoi((sx, sy, 2), np.uint16, (40, 40, 2), seed=sx)
  binary = checker.compress(arr)
  for skip in (False, True):
    _same_cloud(operations._point_cloud_raw(binary, 0, 2, None, skip, 0), checker.point_cloud(binary, 0, -1, None, skip), (sx, skip))


def _stripes(sx, sy, rows=None):
  """Vertical stripes one pixel wide: every column is a component whose contour runs down and back up."""
  x = np.arange(sx).reshape(-1, 1)
  v = np.broadcast_to(1 + (x % 2), (sx, sy)).astype(np.uint8).copy()
  if rows is not None:
    v[:, rows:] = 3
  return v


def test_point_cloud_second_pass_reached_naturally(checker):
  """The first pass's capacities overflow without a switch: a pixel checkerboard (every pixel a one-contour
  component: contours > tab_cap0) and one-pixel stripes (points > raw_cap0; the points of a slice are a lower bound
  on the nodes it keeps).  A volume where only the last slice overflows retries after clean slices."""
  sx, sy = 64, 64
  raw0, tab0 = pc_first_caps(sx, sy)
  x, y = np.meshgrid(np.arange(sx), np.arange(sy), indexing="ij")
  board = (1 + (x + y) % 2).astype(np.uint8)
  sx2, sy2 = 256, 256
  raw2, _ = pc_first_caps(sx2, sy2)
  vols = {
    "checkerboard": np.asfortranarray(np.stack([board, board[::-1]], axis=2)),
    "stripes": np.asfortranarray(np.stack([_stripes(sx2, sy2), _stripes(sx2, sy2)[::-1]], axis=2)),
  }
  last = _voronoi((sx2, sy2, 4), np.uint8, (64, 64, 2), seed=3)
  last[:, :, 3] = _stripes(sx2, sy2)
  vols["last_slice"] = np.asfortranarray(last)
  for name, arr in vols.items():
    binary = checker.compress(arr)
    want = checker.point_cloud(binary, 0, -1, None, False)
    z = np.concatenate([w.reshape(-1, 3)[:, 2] for w in want.values()])
    per_slice = np.bincount(z, minlength=arr.shape[2])
    if name == "checkerboard":
      assert sx * sy > tab0      # one contour per pixel, each a component of its own
      assert np.all(per_slice == sx * sy)
    else:
      assert per_slice[-1] > raw2, (name, per_slice)
      if name == "last_slice":
        assert np.all(per_slice[:-1] <= raw2), per_slice
    _same_cloud(operations._point_cloud_raw(binary, 0, arr.shape[2], None, False, 0), want, name)
    _same_cloud(operations._point_cloud_raw(binary, 0, arr.shape[2], None, True, 0),
                checker.point_cloud(binary, 0, -1, None, True), (name, "skip"))


def _tile_clouds(per_pattern, pattern_of, z0, z1):
  """The point cloud of slices z0..z1-1, slice z holding pattern pattern_of(z): slices are traced alone, so a label's
  points are the per-slice points in z order, with z replaced."""
  out = {}
  for z in range(z0, z1):
    for lab, pts in per_pattern[pattern_of(z)].items():
      p = pts.reshape(-1, 3).copy()
      p[:, 2] = z
      out.setdefault(lab, []).append(p)
  return {k: np.concatenate(v).ravel() for k, v in out.items()}


def test_point_cloud_z_chunks(checker):
  """nz slices (one z-chunk of the first pass), nz + 1 (a second chunk of one slice), and a window starting inside
  the first chunk.  The last slice is dense: its chunk overflows and is traced again, after a clean chunk.  How the
  range was cut is not observable: the counts come from the restated budget."""
  sx, sy = PC_CHUNK_SLICE
  nz = pc_slices_per_chunk(sx, sy)
  raw0, _ = pc_first_caps(sx, sy)
  pats = _voronoi((sx, sy, 3), np.uint8, (256, 256, 1), seed=5)
  dense = pats[:, :, 0].copy()
  dense[:, :1536] = _stripes(sx, 1536)
  pats = np.asfortranarray(np.concatenate([pats, dense[:, :, None]], axis=2))
  pb = checker.compress(pats)
  per = [checker.point_cloud(pb, z, z + 1, None, False) for z in range(4)]
  assert sum(p.size for p in per[3].values()) // 3 > raw0 >= sum(p.size for p in per[0].values()) // 3
  sz = nz + 3
  dev = torch.from_numpy(np.ascontiguousarray(pats.transpose(2, 1, 0))).to(DEV)
  order = [z % 3 for z in range(sz)]
  order[nz] = 3       # the single slice of the second chunk of (0, nz + 1) is the dense one
  vol = dev[torch.tensor(order, device=DEV)]
  binary = ckd.HipBackend(0).encode(vol, (sx, sy, sz))
  del vol, dev
  for z0, z1 in ((0, nz), (0, nz + 1), (2, nz + 3)):
    got = operations._point_cloud_raw(binary, z0, z1, None, False, 0)
    _same_cloud(got, _tile_clouds(per, lambda z: order[z], z0, z1), (z0, z1, nz))


def test_point_cloud_coordinate_truncation(checker):
  """The reference stores (x, y, z) as uint16: a slice 70 000 wide; the slices past 65 535 are in the deep cases."""
  arr = _voronoi((70000, 3, 2), np.uint16, (300, 2, 1), seed=2)
  arr[65530:65545, 1, 1] = 77
  binary = checker.compress(arr)
  want = checker.point_cloud(binary, 0, -1, None, False)
  assert max(int(w.reshape(-1, 3)[:, 0].max()) for w in want.values()) <= 0xFFFF
  _same_cloud(operations._point_cloud_raw(binary, 0, 2, None, False, 0), want, "wide")
  _same_cloud(operations._point_cloud_raw(binary, 1, 2, [77], True, 0), checker.point_cloud(binary, 1, 2, [77], True), "wide sel")


def _squares_slice(sx, sy, n, seed):
  """(uint8 slice on the device, [(label, x0, y0, side)]): labelled squares on background 0, apart and off the border."""
  rng = np.random.default_rng(seed)
  sl = torch.zeros((sy, sx), dtype=torch.uint8, device=DEV)
  sq = []
  cols = 8
  for i in range(n):
    side = 6 + 3 * (i % 7)
    cx, cy = i % cols, i // cols
    x0 = int(cx * (sx // cols) + rng.integers(8, sx // cols - 64))
    y0 = int(cy * (sy // (n // cols + 1)) + rng.integers(8, sy // (n // cols + 1) - 64))
    sl[y0:y0 + side, x0:x0 + side] = i + 1
    sq.append((i + 1, x0, y0, side))
  return sl, sq


def _square_clouds(sq, checker):
  """A square's contour does not depend on where it lies: traced by the checker on a small slice, then moved."""
  out = {}
  for lab, x0, y0, side in sq:
    small = np.zeros((side + 8, side + 8, 1), np.uint8, order="F")
    small[4:4 + side, 4:4 + side, 0] = lab
    w = checker.point_cloud(checker.compress(small), 0, -1, None, True)[lab].reshape(-1, 3).astype(np.int64)
    w[:, 0] += x0 - 4
    w[:, 1] += y0 - 4
    out[lab] = w.astype(np.uint16).ravel()
  return out


@pytest.mark.parametrize("sx,sy", [PC_BIG, PC_LIMIT[0]], ids=["2^29", "limit"])
def test_point_cloud_worst_case_buffers_of_large_slices(sx, sy, checker, monkeypatch):
  """One slice of 2^29 pixels, and the largest slice admitted at this height, through the second pass.
  CKL_CONTOUR_SMALL=64 forces that pass: a dense slice this size is one wavefront walking ~2^28 steps at ~220 ns
  each, minutes for a natural overflow.  Its raw buffer holds pc_raw_worst nodes; before it was sized
  8 sx sy + 16 in 32 bits, 16 entries at 2^29 pixels (`contour buffers overflow`)."""
  assert pc_admitted(sx, sy)
  sl, sq = _squares_slice(sx, sy, 40, seed=sx)
  binary = ckd.HipBackend(0).encode(sl.view(1, sy, sx), (sx, sy, 1))
  del sl
  monkeypatch.setenv("CKL_CONTOUR_SMALL", "64")
  got = operations._point_cloud_raw(binary, 0, 1, None, True, 0)
  monkeypatch.delenv("CKL_CONTOUR_SMALL")
  _same_cloud(got, _square_clouds(sq, checker), (sx, sy))


def test_point_cloud_refuses_slices_above_its_limit():
  """The first slice width past the limit is refused before anything is traced; decoding it still works."""
  sx, sy = PC_LIMIT[1]
  assert not pc_admitted(sx, sy) and (sx + 1) * (sy + 1) < 1 << 30
  sl = torch.zeros((1, sy, sx), dtype=torch.uint8, device=DEV)
  sl[0, 100:120, 200:230] = 3
  binary = ckd.HipBackend(0).encode(sl, (sx, sy, 1))
  del sl
  with pytest.raises(RuntimeError, match="2\\^32 contour nodes"):
    operations._point_cloud_raw(binary, 0, 1, None, True, 0)
  assert crackle_amd.voxel_counts(binary) == {0: sx * sy - 600, 3: 600}


# ---------------------------------------------------------------------------------------------------------------------
# deep volumes
DEEP = [65535, 65536, 70001]


def _deep(sx, sy, sz):
  x, y, z = np.meshgrid(np.arange(sx), np.arange(sy), np.arange(sz), indexing="ij")
  v = 1 + (x // 2 + 3 * y + z // 3) % 5 + 5 * ((z // 7) % 3)
  v[(x == 1) & (y == 1) & (z % 1000 == 999)] = 40
  return np.asfortranarray(v.astype(np.uint16))


DEEP_CASES = [(sz, 4, 4) for sz in DEEP] + [(DEEP[-1], 5, 3)]      # slices of the strip decoder (sx % 4 == 0), and not


@pytest.mark.parametrize("sz,sx,sy", DEEP_CASES, ids=[f"{a}-{b}x{c}" for a, b, c in DEEP_CASES])
def test_deep_volumes(sz, sx, sy, checker):
  """More than 65 535 slices.  The general pipeline, k_run_stats, k_vcg and the contour kernels take a slice per
  workgroup or per blockIdx.y.  An MI355X reports maxGridSize = (2^31 - 1, 65 536, 65 536): 70 001 slices on
  blockIdx.y are past the reported y limit, yet the runtime launches them and every result below is checked."""
  print("maxGridSize", _max_grid(), "slices", sz)
  assert _max_grid()[0] >= sz
  arr = _deep(sx, sy, sz)
  binary = checker.compress(arr, parallel=16)
  assert crackle_amd.compress(arr) == binary
  assert np.array_equal(crackle_amd.decompress(binary), arr)
  got = crackle_amd.decompress_range(binary, sz - 3, sz)
  assert np.array_equal(got, arr[:, :, sz - 3:]), "far window"
  check_stats(binary, arr, checker, sz)
  v6 = crackle_amd.voxel_connectivity_graph(binary, 6)
  assert np.array_equal(v6, checker.voxel_connectivity_graph(binary, 6, parallel=16))
  _same_cloud(operations._point_cloud_raw(binary, 0, sz, None, False, 0), checker.point_cloud(binary, 0, -1, None, False), sz)
  r = crackle_amd.reencode(binary, 3)
  assert r == checker.reencode(binary, 3, parallel=16)
  assert crackle_amd.reencode(r, 0) == binary


# ---------------------------------------------------------------------------------------------------------------------
# label statistics
def _columns(sx, sy, n):
  """A slice of one-pixel columns with exactly n components: labels 1 + x % 5, every column from n - 1 on alike."""
  x = np.minimum(np.arange(sx), n - 1)
  return np.broadcast_to((1 + x % 5).reshape(-1, 1), (sx, sy)).astype(np.uint16)


def test_label_stats_lds_and_run_by_run(checker):
  """Slices of fit - 1, fit and fit + 1 components in one volume: the first two accumulate in LDS, the third merges
  run by run (decided per slice).  Labels span all slices, so both kinds merge into the same labels.  Which kind ran
  is not observable; the component counts per slice are asserted from the volume."""
  fit = stats_fit()
  sx, sy = fit + 1, 3
  ns = [fit - 1, fit, fit + 1, fit]
  arr = np.asfortranarray(np.stack([_columns(sx, sy, n) for n in ns], axis=2))
  _check_stats_streams(arr, ns, checker)
  arr[5, 1, 2] = 9
  _check_stats_streams(arr, [], checker)


def test_label_stats_odd_component_count(checker):
  """max_comp = 101: LDS capacity rounded up to 102."""
  arr = np.asfortranarray(np.stack([_columns(200, 4, n) for n in (STATS_MAX_ODD, 40)], axis=2))
  _check_stats_streams(arr, [STATS_MAX_ODD, 40], checker)


def _check_stats_streams(arr, ncomp, checker):
  for z, n in enumerate(ncomp):      # components per slice: one per run of equal columns
    row = arr[:, 0, z]
    assert 1 + int(np.count_nonzero(row[1:] != row[:-1])) == n, (z, n)
  for kw in (dict(), dict(allow_pins=True), dict(markov_model_order=2)):
    binary = checker.compress(arr, **kw)
    assert crackle_amd.compress(arr, **kw) == binary, kw
    check_stats(binary, arr, checker, kw)


# ---------------------------------------------------------------------------------------------------------------------
# voxel connectivity graph
def _vcg_volumes():
  hbm = _hbm_row_words()
  vols = [
    ("voronoi_1", lambda: _voronoi((37, 41, 1), np.uint32, (6, 6, 1), 1)),
    ("voronoi_2", lambda: _voronoi((37, 41, 2), np.uint32, (6, 6, 1), 2)),
    ("noise_1", lambda: synth.random_labels((33, 20, 1), np.uint8, seed=4, high=3)),       # PERMISSIBLE
    ("noise_2", lambda: synth.random_labels((33, 20, 2), np.uint8, seed=5, high=3)),
    ("c_order_2", lambda: np.ascontiguousarray(_voronoi((30, 17, 2), np.uint16, (5, 5, 1), 3))),
    ("raster_16416x1024", lambda: _voronoi((16416, 1024, 1), np.uint16, (1000, 7, 1), 4)),
    ("general_16416x1025", lambda: _voronoi((16416, 1025, 2), np.uint16, (1000, 7, 1), 5)),
    ("lds_raster", lambda: _voronoi(((hbm - 1) * 32, 3, 2), np.uint16, (1000, 2, 1), 6)),
    ("hbm_raster", lambda: _voronoi((hbm * 32 - 31, 3, 2), np.uint16, (1000, 2, 1), 7)),
  ]
  return vols


@pytest.mark.parametrize("idx", range(9))
def test_vcg(idx, checker):
  name, make = _vcg_volumes()[idx]
  arr = make()
  binary = checker.compress(arr, parallel=16)
  h = crackle_amd.header(binary)
  if name.startswith("noise"):
    assert h.crack_format == crackle_amd.CrackFormat.PERMISSIBLE, name
  if name.startswith("c_order"):
    assert not h.fortran_order
  for conn in (4, 6):
    got = crackle_amd.voxel_connectivity_graph(binary, conn)
    assert np.array_equal(got, checker.voxel_connectivity_graph(binary, conn, parallel=16)), (name, conn)


# ---------------------------------------------------------------------------------------------------------------------
# reencode at the §6a edge shapes
def _reencode_volumes():
  hbm = _hbm_row_words()
  out = [(f"w{sx}", (lambda sx=sx: _voronoi((sx, 37, 3), np.uint16, (5, 5, 2), sx))) for sx in (1, 2, 3, 31, 32, 33, 254, 255, 256)]
  out += [
    ("h65534", lambda: _voronoi((8, 65534, 2), np.uint8, (4, 32, 1), 1)),
    ("h65535", lambda: _voronoi((8, 65535, 2), np.uint8, (4, 32, 1), 2)),
    ("hbm_raster", lambda: _voronoi((hbm * 32 - 31, 3, 2), np.uint16, (1000, 2, 1), 7)),
    ("walk_fast", lambda: synth.random_labels((256, 256, 3), np.uint8, seed=4, high=2)),
    ("walk_compiled", lambda: synth.random_labels((1024, 1024, 3), np.uint8, seed=4, high=2)),
  ]
  return out


@pytest.mark.parametrize("idx", range(14))
def test_reencode_edges(idx, checker):
  name, make = _reencode_volumes()[idx]
  arr = make()
  b0 = checker.compress(arr, parallel=16)
  assert crackle_amd.compress(arr) == b0, name
  for k in (1, 5, 13):
    bk = crackle_amd.reencode(b0, k)
    if k < 13:      # the checker takes seconds to build an order-13 model: once per case, in its reencode
      assert bk == checker.compress(arr, markov_model_order=k, parallel=16), (name, k)
    assert bk == checker.reencode(b0, k, parallel=16), (name, k)
    assert crackle_amd.reencode(bk, 0) == b0, (name, k)


# ---------------------------------------------------------------------------------------------------------------------
# mode_pooling_2x2x1
def _np_pool(arr):
  """operations.hpp:1254-1290: a == b -> a, a == c -> a, b == c -> b, else d; an odd last column or row copies a."""
  sx, sy, sz = arr.shape
  ox, oy = (sx + 1) // 2, (sy + 1) // 2
  out = arr[0::2, 0::2, :].copy()
  full_x, full_y = sx // 2, sy // 2
  a = arr[0:2 * full_x:2, 0:2 * full_y:2]
  b = arr[1:2 * full_x:2, 0:2 * full_y:2]
  c = arr[0:2 * full_x:2, 1:2 * full_y:2]
  d = arr[1:2 * full_x:2, 1:2 * full_y:2]
  out[:full_x, :full_y] = np.where(a == b, a, np.where(a == c, a, np.where(b == c, b, d)))
  assert out.shape == (ox, oy, sz)
  return np.asfortranarray(out)


def _pool_shapes(itemsize):
  p = 16 // itemsize
  return [(1, 1), (1, 3), (2, 2), (3, 1), (3, 2), (2 * p - 2, 5), (2 * p - 1, 5), (2 * p, 3), (2 * p + 2, 4), (2 * p + 3, 3)]


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_mode_pooling_edges(dt, checker):
  """Widths whose pooled width (sx + 1) // 2 crosses the encoder's label-plane fast path (P = 16 / itemsize)."""
  p = 16 // np.dtype(dt).itemsize
  shapes = _pool_shapes(np.dtype(dt).itemsize)
  assert {((sx + 1) // 2) % p == 0 and (sx + 1) // 2 >= p for sx, _ in shapes} == {True, False}
  for sx, sy in shapes:
    arr = synth.random_labels((sx, sy, 4), dt, seed=sx * 31 + sy, high=4)
    for kw in (dict(), dict(allow_pins=True)):
      binary = checker.compress(arr, **kw)
      got = operations._mode_pooling_slices(binary)
      assert got == checker.mode_pooling_2x2x1(binary), (sx, sy, kw)
      assert operations._mode_pooling_slices(binary, 1, 3) == checker.mode_pooling_2x2x1(binary, 1, 3), (sx, sy, kw)
      # slices pooled alone may pick different crack formats, which zstack refuses like the reference
      pooled = np.concatenate([crackle_amd.decompress(b) for b in got], axis=2)
      assert np.array_equal(pooled, _np_pool(arr)), (sx, sy, kw)
      if len({crackle_amd.header(b).crack_format for b in got}) == 1:
        assert np.array_equal(crackle_amd.decompress(crackle_amd.mode_pooling_2x2x1(binary)), pooled), (sx, sy, kw)


# ---------------------------------------------------------------------------------------------------------------------
# array_equal and check
def _eq_volumes():
  hbm = _hbm_row_words()
  return [("general", lambda: _voronoi((37, 300, 3), np.uint32, (9, 7, 2), 37)),
          ("hbm_raster", lambda: _voronoi((hbm * 32 - 31, 3, 2), np.uint16, (1000, 2, 1), 7))]


@pytest.mark.parametrize("idx", range(2))
def test_array_equal_and_check(idx, checker):
  name, make = _eq_volumes()[idx]
  arr = make()
  sx, sy, sz = arr.shape
  encs = [checker.compress(arr), checker.compress(arr, allow_pins=True), checker.compress(arr, markov_model_order=4)]
  for i in range(3):
    for j in range(3):
      assert crackle_amd.array_equal(encs[i], encs[j]) and checker.array_equal(encs[i], encs[j]), (name, i, j)
  # one voxel changed to another label of the volume: first, last, and one on a seam between rows 0 and 1
  for pos in ((0, 0, 0), (sx - 1, sy - 1, sz - 1), (sx // 2, 1, 1)):
    other = arr.copy(order="F")
    labs = np.unique(arr)
    other[pos] = labs[0] if arr[pos] != labs[0] else labs[-1]
    for b2 in (checker.compress(other), checker.compress(other, allow_pins=True)):
      assert np.array_equal(crackle_amd.labels(b2), crackle_amd.labels(encs[0])), (name, pos)      # the device decides
      for b1 in encs:
        assert not crackle_amd.array_equal(b1, b2), (name, pos)
        assert not checker.array_equal(b1, b2), (name, pos)
  # one slice's crack code damaged: check() names exactly that slice
  for b in encs:
    h = crackle_amd.header(b)
    hb = h.header_bytes
    lens = [int.from_bytes(b[hb + 4 * z:hb + 4 * z + 4], "little") for z in range(h.sz)]
    z = h.sz - 1
    off = hb + h.grid_index_bytes + h.num_label_bytes + h.markov_model_bytes + sum(lens[:z])
    bad = bytearray(b)
    bad[off + lens[z] // 2] ^= 0x5A
    rep = crackle_amd.check(bytes(bad))
    assert rep["header"] and rep["crack_index"] and rep["labels"], (name, rep)
    assert rep["z"] == [z], (name, rep)
    assert not crackle_amd.ok(bytes(bad)) and crackle_amd.ok(b)
