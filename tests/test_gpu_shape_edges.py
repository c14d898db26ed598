"""GPU tests on both sides of the plan thresholds: the geometry limits by which the host code picks a kernel.

Where these thresholds live:
- the decoder's front end: crack records (k_crack_match), the rasterising kernel (k_decode_cracks) or the general
  run pipeline;
- its strip kernel: k_strip_ccl2 against k_strip_ccl;
- the general pipeline's raster: LDS bands against zeroed planes in HBM (the `memset` stage);
- the encoder's label-plane fast path, its label stream, its walk and its pin dedup tiers;
- the coordinate widths of the format.

Every case asserts which side it reached, so a case that drifts off its edge fails instead of covering nothing.  On
the decoder this is the stage names of HipDecodeSession.stages(), checked against `plan()`, a restatement of the
host rule in ckl_decode.hip (decoder_build / decoder_run).  On the encoder it is HipBackend.walk_paths() or a
predicate restated from ckl_encode.hip.  Then the encoder's bytes must equal the checker's (the compiled reference
where it was built), and the decoder must give the input back: the whole volume, a z-window and `label=`.  Where a
case is on the strip path, the general pipeline (CKL_DECODE_GENERAL=1) decodes it a second time.

Shapes are natural: a CKL_* switch only appears where it is named in the case, with the reason."""
import ctypes as C

import numpy as np
import pytest
import torch

import crackle_amd
from crackle_amd import _lib, synth
from crackle_amd import distributed as ckd

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TORCH_DT = {1: torch.uint8, 2: torch.uint16, 4: torch.uint32, 8: torch.uint64}
FLAT = 0
PERMISSIBLE = 1

# constants of the plan (ckl_strips.hpp, ckl_crack_records.hpp, ckl_decode.hip)
K_STRIP_WORDS = 1024
K_STRIP_CAP = 2560
K_MAX_STRIPS = 1024
K_REC_MAX_STRIPS = 512
K_REC_MAX_DIM = 65534
K_RESOLVE_CAP = 0xFFFF
SLOW = {"k_decode_cracks", "k_run_index", "k_run_union_strips", "k_run_assign", "k_paint_runs"}


def _bw(x):
  return 1 if x <= 0xFF else 2 if x <= 0xFFFF else 4 if x <= 0xFFFFFFFF else 8


def _max_lds():
  p = torch.cuda.get_device_properties(0)
  return int(getattr(p, "shared_memory_per_block", 0) or 160 * 1024)


def _n_cus():
  return int(torch.cuda.get_device_properties(0).multi_processor_count)


def crack_lds_seg_bytes(n):
  return (n + 2) * 8


def crack_lds_bytes(n):
  return crack_lds_seg_bytes(n) + n * 8 + n * 8 + n * 4 + (n // 7 + 48) * 2 + n + 16


def lds_controls():
  """(capacity of k_decode_cracks' LDS control tables, its dynamic LDS bytes): decoder_new."""
  budget = max(_max_lds() - 4096, 0)
  n = 5120
  while n > 64 and crack_lds_bytes(n) > budget:
    n -= 64
  if crack_lds_bytes(n) > budget:
    n = 0
  return min(n, 32000), max(crack_lds_bytes(n), budget & ~15)


def hbm_raster_row_words():
  """The fewest plane words per row for which k_decode_cracks rasterises into zeroed planes in HBM."""
  n, lds = lds_controls()
  return (lds - crack_lds_seg_bytes(n)) // 8 + 1


def plan(binary, z0=0, z1=None, env=None):
  """The decoder's plan for the stream, restated from decoder_build / decoder_run / launch_strips."""
  env = env or {}
  h = crackle_amd.header(binary)
  z1 = h.sz if z1 is None else z1
  ns = z1 - z0
  sx, sy = h.sx, h.sy
  hb = h.header_bytes
  lens = [int.from_bytes(binary[hb + 4 * z:hb + 4 * z + 4], "little") for z in range(h.sz)]
  off = hb + h.grid_index_bytes + h.num_label_bytes + h.markov_model_bytes + sum(lens[:z0])
  est = 0.0
  for z in range(z0, z1):
    n = lens[z]
    idx = int.from_bytes(binary[off:off + 4], "little") if n >= 4 else 0
    payload = n - 4 - idx if n >= 4 + idx else 0
    est += payload * 8 / 1.4 if h.markov_model_order else payload * 4.0
    off += n
  row_words = (sx + 31) // 32
  strip_rows = max(1, K_STRIP_WORDS // row_words)
  if h.crack_format != PERMISSIBLE and ns:
    runs_per_row = 1.0 + 0.5 * est / (float(ns) * sy)
    strip_rows = max(1, min(strip_rows, int(0.7 * K_STRIP_CAP / runs_per_row)))
  if "CKL_CCL_ROWS" in env:
    strip_rows = max(1, min(K_STRIP_WORDS // row_words, max(1, int(env["CKL_CCL_ROWS"]))))
  nstrips = (sy + strip_rows - 1) // strip_rows
  strips = (h.fortran_order and sx % 4 == 0 and row_words <= K_STRIP_WORDS and nstrips <= K_MAX_STRIPS
            and sx * sy < 0xFFFF0000 and "CKL_DECODE_GENERAL" not in env)
  records = strips and sx <= K_REC_MAX_DIM and sy <= K_REC_MAX_DIM and nstrips <= K_REC_MAX_STRIPS and "CKL_DECODE_RASTER" not in env
  v2 = records and row_words in (4, 8, 16, 32, 64, 128, 256, 512)
  n, lds = lds_controls()
  lds_raster = lds >= crack_lds_seg_bytes(n) + 8 * row_words
  return dict(strips=strips, records=records, v2=v2, lds_raster=lds_raster, strip_rows=strip_rows, nstrips=nstrips,
              row_words=row_words, flat=h.label_format == FLAT, xw=_bw(sx + 1), yw=_bw(sy + 1))


def check_path(names, p, what=""):
  """The stage names are the ones `p` (plan()) predicts."""
  if p["strips"]:
    front = "k_crack_match" if p["records"] else "k_decode_cracks"
    ccl = "k_strip_ccl2" if p["v2"] else "k_strip_ccl"
    assert names[:3] == [front, ccl, "k_slice_resolve"], (what, names, p)
    assert names[-1] == "k_paint_strips" and not (SLOW - {"k_decode_cracks"}) & set(names), (what, names, p)
  else:
    head = [] if p["lds_raster"] else ["memset"]
    assert names[:len(head) + 1] == head + ["k_decode_cracks"], (what, names, p)
    assert "k_paint_runs" in names and not {"k_crack_match", "k_strip_ccl", "k_strip_ccl2"} & set(names), (what, names, p)


def decode(binary, z0=0, z1=None, label=None):
  """(F-ordered numpy volume, stage names) of one decode on the device."""
  h = crackle_amd.header(binary)
  z1 = h.sz if z1 is None else z1
  s = ckd.HipDecodeSession(binary, z0, z1, 0)
  try:
    out = torch.empty((z1 - z0, h.sy, h.sx), dtype=torch.uint8 if label is not None else TORCH_DT[h.data_width], device=DEV)
    s.run(out, label)
    names = [n for n, _ in s.stages()]
  finally:
    s.close()
  got = synth.as_numpy_f(out)
  return (got.view(bool) if label is not None else got), names


def _set_env(monkeypatch, env):
  for k in ("CKL_DECODE_GENERAL", "CKL_CCL_ROWS", "CKL_DECODE_RASTER"):
    monkeypatch.delenv(k, raising=False)
  for k, v in (env or {}).items():
    monkeypatch.setenv(k, v)


def roundtrip(binary, arr, monkeypatch, window=None, labels=(), env=None, what=""):
  """Decodes the whole volume, a z-window and label images, each on its predicted path; the strip path also
  through the general pipeline.  Returns the plan of the whole decode."""
  env = dict(env or {})
  p = plan(binary, env=env)
  runs = [env]
  if p["strips"]:
    runs.append(dict(env, CKL_DECODE_GENERAL="1"))
  for e in runs:
    _set_env(monkeypatch, e)
    pe = plan(binary, env=e)
    got, names = decode(binary)
    assert np.array_equal(got, arr), (what, e)
    check_path(names, pe, (what, e))
    if window:
      z0, z1 = window
      got, names = decode(binary, z0, z1)
      assert np.array_equal(got, arr[:, :, z0:z1]), (what, e, window)
      check_path(names, plan(binary, z0, z1, env=e), (what, e, window))
    for lab in labels:
      got, names = decode(binary, label=int(lab))
      assert np.array_equal(got, arr == lab), (what, e, lab)
      check_path(names, pe, (what, e, lab))
  _set_env(monkeypatch, None)
  return p


def _np_stats(arr):
  """{label: (count, centroid, box)} from numpy: centroids are exact int64 coordinate sums divided once in float64."""
  sx, sy, sz = arr.shape
  flat = arr.reshape(-1, order="F")
  u, inv = np.unique(flat, return_inverse=True)
  cnt = np.bincount(inv)
  idx = np.arange(flat.size, dtype=np.int64)
  x, y, z = idx % sx, (idx // sx) % sy, idx // (sx * sy)
  order = np.argsort(inv, kind="stable")
  starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])
  out = {}
  sums = [np.add.reduceat(c[order], starts) for c in (x, y, z)]      # exact: int64
  mins = [np.minimum.reduceat(c[order], starts) for c in (x, y, z)]
  maxs = [np.maximum.reduceat(c[order], starts) for c in (x, y, z)]
  for i, lab in enumerate(u.tolist()):
    out[int(lab)] = (int(cnt[i]), np.array([np.float64(s[i]) / np.float64(cnt[i]) for s in sums]),
                     [int(m[i]) for m in mins] + [int(m[i]) for m in maxs])
  return out


def check_consumers(binary, arr, vcg=False):
  want = _np_stats(arr)
  counts = crackle_amd.voxel_counts(binary)
  assert counts == {k: v[0] for k, v in want.items()}
  cents = crackle_amd.centroids(binary)
  assert sorted(cents) == sorted(want)
  for k, (_, c, _) in want.items():
    assert cents[k].dtype == np.float64 and np.array_equal(cents[k], c), (k, cents[k], c)
  boxes = crackle_amd.bounding_boxes(binary, no_slice_conversion=True)
  assert {k: [int(v) for v in b] for k, b in boxes.items()} == {k: v[2] for k, v in want.items()}
  if vcg:
    v = crackle_amd.voxel_connectivity_graph(binary, 6)
    assert np.array_equal((v[:-1] & 0x01) != 0, arr[:-1] == arr[1:])
    assert np.array_equal((v[1:] & 0x02) != 0, arr[1:] == arr[:-1])
    assert np.array_equal((v[:, :-1] & 0x04) != 0, arr[:, :-1] == arr[:, 1:])
    assert np.array_equal((v[:, 1:] & 0x08) != 0, arr[:, 1:] == arr[:, :-1])
    assert np.array_equal((v[:, :, :-1] & 0x10) != 0, arr[:, :, :-1] == arr[:, :, 1:])


def _labels(arr, k=2):
  u = np.unique(arr)
  return [int(u[0]), int(u[len(u) // 2])][:k]


# ---------------------------------------------------------------------------------------------------------------------
# A. width sweep
WIDTHS = [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 97, 100, 127, 128, 129, 132, 252, 254, 255, 256]
PIN_WIDTHS = {4, 5, 17, 32, 33, 100, 129, 255, 256}
DTYPES = [np.uint8, np.uint16, np.uint32, np.uint64]
SHAPES_A = [(sx, 37) for sx in WIDTHS] + [(36, sy) for sy in (254, 255, 256)]


def planes_fast(sx, itemsize):
  """The encoder's label-plane fast path (ckl_encode.hip: planes_pass), for a 16-byte aligned volume."""
  p = 16 // itemsize
  return sx >= p and sx % p == 0


def _sweep_volume(sx, sy, dt):
  arr = synth.as_numpy_f(synth.voronoi_labels((sx, sy, 3), dt, seed=sx * 7 + sy, cell=(5, 5, 2)))
  arr[sx // 2, :, 1:] = 7      # a stripe one pixel wide through two slices
  return np.asfortranarray(arr)


def test_width_sweep_straddles_every_threshold():
  """Each threshold of the sweep has shapes on both of its sides."""
  rw = [((sx + 31) // 32) for sx, _ in SHAPES_A]
  sides = {
    "strip sx % 4": {sx % 4 == 0 for sx, _ in SHAPES_A},
    "k_strip_ccl2 rows": {r in (4, 8, 16, 32, 64, 128, 256, 512) for r, (sx, _) in zip(rw, SHAPES_A) if sx % 4 == 0},
    "boc x width": {_bw(sx + 1) for sx, _ in SHAPES_A},
    "boc y width": {_bw(sy + 1) for _, sy in SHAPES_A},
  }
  for dt in DTYPES:
    sides[f"planes fast {np.dtype(dt).name}"] = {planes_fast(sx, np.dtype(dt).itemsize) for sx, _ in SHAPES_A}
  for name, s in sides.items():
    assert len(s) == 2, name


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("sx,sy", SHAPES_A, ids=[f"{a}x{b}" for a, b in SHAPES_A])
def test_width_sweep(sx, sy, dt, checker, monkeypatch):
  arr = _sweep_volume(sx, sy, dt)
  opts = [dict(markov_model_order=0), dict(markov_model_order=3)]
  if sx in PIN_WIDTHS:
    opts.append(dict(allow_pins=True))
  for kw in opts:
    want = checker.compress(arr, **kw)
    assert crackle_amd.compress(arr, **kw) == want, kw
    p = roundtrip(want, arr, monkeypatch, window=(1, 3), labels=_labels(arr) + [7], what=kw)
    assert p["strips"] == (sx % 4 == 0) and p["xw"] == _bw(sx + 1) and p["yw"] == _bw(sy + 1)
    if p["strips"]:
      assert p["records"] and p["v2"] == (p["row_words"] in (4, 8)), p


# ---------------------------------------------------------------------------------------------------------------------
# B. strip count and row width (one row per strip above 512 plane words)
def _dev_volume(shape, dt, cell, seed=3):
  return synth.voronoi_labels(shape, dt, seed=seed, cell=cell, device=DEV)


def _slanted(shape, dt, period):
  """Slanted bands `period` pixels wide: every row crosses the same number of boundaries.  A strip of one row
  holds one strip component per band, and a slice's crack records spread evenly over its strips; the rows of a
  Voronoi volume instead meet its cells' horizontal edges in a few strips, which overflow their record lists and
  hand the session over to the rasterising kernel (a capacity hand-over, not what these cases are about)."""
  sx, sy, sz = shape
  x = torch.arange(sx, device=DEV).view(1, 1, -1)
  y = torch.arange(sy, device=DEV).view(1, -1, 1)
  z = torch.arange(sz, device=DEV).view(-1, 1, 1)
  return (1 + ((x + y + 3 * z) // period) % 250).to(TORCH_DT[np.dtype(dt).itemsize])


def _grid(shape, dt, cell):
  """A regular grid of cells: the same runs in every row, so the strip heights the plan estimates hold."""
  sx, sy, sz = shape
  x = torch.arange(sx, device=DEV).view(1, 1, -1)
  y = torch.arange(sy, device=DEV).view(1, -1, 1)
  z = torch.arange(sz, device=DEV).view(-1, 1, 1)
  return (1 + (x // cell[0] + 2 * (y // cell[1]) + 5 * z) % 250).to(TORCH_DT[np.dtype(dt).itemsize])


HBM = hbm_raster_row_words() if torch.cuda.is_available() else 0
# name, (sx, sy, sz), expected front end ("records", "raster", "general"), strip kernel, HBM raster
CASES_B = [
  ("rec_16416x512", (16416, 512, 1), "records", "k_strip_ccl", False),
  ("raster_16416x513", (16416, 513, 1), "raster", "k_strip_ccl", False),
  ("raster_16416x1024", (16416, 1024, 1), "raster", "k_strip_ccl", False),
  ("general_16416x1025", (16416, 1025, 1), "general", None, False),
  ("rec_v2_16384", (16384, 64, 2), "records", "k_strip_ccl2", False),
  ("rec_v1_32768", (32768, 64, 2), "records", "k_strip_ccl", False),
  ("general_32772", (32772, 64, 2), "general", None, False),
  ("lds_raster_1row", ("hbm-1", 1, 2), "general", None, False),
  ("lds_raster_3rows", ("hbm-1", 3, 1), "general", None, False),
  ("hbm_raster_1row", ("hbm", 1, 2), "general", None, True),
  ("hbm_raster_3rows", ("hbm", 3, 1), "general", None, True),
]


def _front(p):
  return "records" if p["records"] else "raster" if p["strips"] else "general"


@pytest.mark.parametrize("name,shape,front,ccl,hbm", CASES_B, ids=[c[0] for c in CASES_B])
def test_strip_count_and_row_width(name, shape, front, ccl, hbm, checker, monkeypatch):
  sx, sy, sz = shape
  if sx == "hbm":
    sx = HBM * 32 - 31      # the first width of HBM words per row
  elif sx == "hbm-1":
    sx = (HBM - 1) * 32     # the last width of one word fewer
  arr = synth.as_numpy_f(_slanted((sx, sy, sz), np.uint16, 1000))
  want = checker.compress(arr, parallel=16)
  assert crackle_amd.compress(arr) == want, name
  p = plan(want)
  assert _front(p) == front, (name, p)
  if ccl:
    assert p["v2"] == (ccl == "k_strip_ccl2"), (name, p)
  if p["strips"]:
    assert p["strip_rows"] == 1 or name == "rec_v2_16384", p
  assert (not p["lds_raster"]) == hbm, (name, p)
  roundtrip(want, arr, monkeypatch, window=(1, 2) if sz > 1 else None, labels=_labels(arr, 1), what=name)
  if name in ("raster_16416x1024", "general_16416x1025", "hbm_raster_3rows"):
    check_consumers(want, arr)


# ---------------------------------------------------------------------------------------------------------------------
# C. slice height and the 16-bit coordinates of the crack records
# name, (sx, sy, sz), front end
CASES_C = [
  ("rec_h65534", (8, 65534, 2), "records"),
  ("raster_h65535", (8, 65535, 2), "raster"),
  ("raster_h65536", (4, 65536, 3), "raster"),
  ("raster_h131075", (8, 131075, 2), "raster"),
  ("general_w65534", (65534, 3, 2), "general"),
  ("general_w65535", (65535, 2, 2), "general"),
  ("general_w65536", (65536, 4, 2), "general"),
]


@pytest.mark.parametrize("name,shape,front", CASES_C, ids=[c[0] for c in CASES_C])
def test_slice_height_and_coordinate_width(name, shape, front, checker, monkeypatch):
  sx, sy, sz = shape
  if sx <= 8:
    arr = synth.as_numpy_f(_grid(shape, np.uint16, (4, 32)))
  else:
    arr = synth.as_numpy_f(_dev_volume(shape, np.uint16, cell=(64, 2, 1), seed=sy))
  want = checker.compress(arr, parallel=16)
  assert crackle_amd.compress(arr) == want, name
  p = plan(want)
  assert _front(p) == front, (name, p)
  assert p["xw"] == _bw(sx + 1) and p["yw"] == _bw(sy + 1)
  assert (p["yw"] if sx <= 8 else p["xw"]) == (2 if max(sx, sy) < 65535 else 4), p
  roundtrip(want, arr, monkeypatch, window=(1, 2), labels=_labels(arr), what=name)
  if front != "general":
    # strips of 1000 rows: the records' division by multiply (strip_magic) and the strips' ragged last rows
    # on a strip height that is not a power of two, named here because the content decides the natural height
    env = {"CKL_CCL_ROWS": "1000"}
    pe = roundtrip(want, arr, monkeypatch, window=(0, 1), env=env, what=(name, env))
    assert pe["strip_rows"] == 1000 and _front(pe) == front
  check_consumers(want, arr, vcg=sx * sy * sz <= (1 << 20))


# ---------------------------------------------------------------------------------------------------------------------
# D. slice count against the CU count
def test_slices_against_cus(checker):
  """`few = nslices <= n_cus` gives k_crack_match and k_slice_resolve a CU's LDS each; with more slices two share it
  and the resolver's table escalates to a CU's LDS for slices of more than resolve_cap / 2 components."""
  n = _n_cus()
  shape = (512, 512, n + 8)
  vol = _dev_volume(shape, np.uint32, cell=(5, 5, 2), seed=9)
  be = ckd.HipBackend(0)
  binary = be.encode(vol, shape)
  assert binary == checker.compress(synth.as_numpy_f(vol), parallel=16)
  # components per slice against the shared and the whole-CU resolver table
  h = crackle_amd.header(binary)
  sec = binary[h.header_bytes + h.grid_index_bytes:][:h.num_label_bytes]
  nu = int.from_bytes(sec[0:8], "little")
  p0 = 8 + h.stored_data_width * nu
  most = max(int.from_bytes(sec[p0 + 4 * z:p0 + 4 * z + 4], "little") for z in range(h.sz))
  lds = _max_lds()
  shared = min(K_RESOLVE_CAP, (lds // 2 - 6144 - (K_MAX_STRIPS + 64) * 4) // 4)
  alone = min(K_RESOLVE_CAP, (lds - 8192 - (K_MAX_STRIPS + 64) * 4) // 4)
  assert shared < 2 * most <= alone, (most, shared, alone)
  fast = ["k_crack_match", "k_strip_ccl2", "k_slice_resolve", "k_paint_strips"]
  for z0, z1 in ((0, n), (0, n + 1), (3, n + 3), (7, n + 8), (0, n + 8)):
    s = be.open_decoder(binary, z0, z1)
    out = torch.empty((z1 - z0, 512, 512), dtype=torch.uint32, device=DEV)
    s.run(out)
    names = [m for m, _ in s.stages()]
    s.close()
    assert names == fast, (z0, z1, names)
    assert torch.equal(out.view(torch.int32), vol[z0:z1].view(torch.int32)), (z0, z1)


# ---------------------------------------------------------------------------------------------------------------------
# E. pin dedup depth tiers: 1 / 2 / 4 / 8 / 16 label registers per lane up to 64 / 128 / 256 / 512 / 1024 slices
TIERS = [64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025]


def _tier_volume(sx, sy, sz):
  """Every column changes label at every slice (sz labels: a tier's table is full at its top); columns two apart
  share labels one slice apart, so the labels' components meet in pins."""
  x, y, z = np.meshgrid(np.arange(sx), np.arange(sy), np.arange(sz), indexing="ij")
  return np.asfortranarray((1 + (z + x // 2 + 3 * y) % 4001).astype(np.uint16))


@pytest.mark.parametrize("sx", [8, 9])
@pytest.mark.parametrize("sz", TIERS)
def test_pin_dedup_tiers(sz, sx, checker, monkeypatch):
  arr = _tier_volume(sx, 5, sz)
  cols = arr.reshape(sx * 5, sz)
  assert all(len(np.unique(c)) == sz for c in cols)      # the column's table holds sz labels
  tier = next((t for t in (64, 128, 256, 512, 1024) if sz <= t), None)
  assert tier is None or sz in (tier, tier // 2 + 1), (sz, tier)      # at the top of its tier or just past the one below
  want = checker.compress(arr, allow_pins=True)
  assert crackle_amd.compress(arr, allow_pins=True) == want, sz
  roundtrip(want, arr, monkeypatch, window=(sz // 2, sz // 2 + 3), labels=[int(arr[0, 0, 0]), int(arr[3, 2, sz - 1])], what=sz)


# ---------------------------------------------------------------------------------------------------------------------
# F. encoder plan
@pytest.mark.parametrize("sy", [1536, 1540])
def test_label_stream_threshold(sy, checker):
  """The label stream starts in front of the graph kernel for slices above 1536 x 1536 pixels (ckl_encoder_run).
  Which side ran cannot be seen from outside the encoder (no stage table, and walk_paths() is the same on both): the
  case asserts only that its shapes straddle the rule as restated here, then bytes and the round trip on each side."""
  shape = (1536, sy, 2)
  assert (shape[0] * shape[1] > 1536 * 1536) == (sy > 1536)
  vol = _dev_volume(shape, np.uint32, cell=(24, 24, 2), seed=sy)
  be = ckd.HipBackend(0)
  binary = be.encode(vol, shape)
  assert sum(be.walk_paths()) == 2
  assert binary == checker.compress(synth.as_numpy_f(vol), parallel=16)
  s = be.open_decoder(binary, 0, 2)
  out = torch.empty_like(vol)
  s.run(out)
  s.close()
  assert torch.equal(out.view(torch.int32), vol.view(torch.int32))


# name, volume, slices walked by the hand-scheduled loop, slices walked by the compiled one (counts measured once on
# an MI355X and pinned here).  Noise of two labels: 256 x 256 slices stay on the hand-scheduled loop; 1024 x 1024
# slices have more than 65 535 walk events, more than the fast walk's stack entries can name.
# Not covered: whether the compiled walk keeps its tables in LDS (nn < 16384 nodes, ckl_trail.hpp) or in HBM;
# walk_paths() reports the same count for both.
def _walk_fast():
  return synth.random_labels_device((256, 256, 3), np.uint8, seed=4, high=2, device=DEV)


def _walk_compiled():
  return synth.random_labels_device((1024, 1024, 3), np.uint8, seed=4, high=2, device=DEV)


WALKS = [("fast", _walk_fast, 3, 0), ("compiled", _walk_compiled, 0, 3)]


@pytest.mark.parametrize("name,make,n_fast,n_compiled", WALKS, ids=[w[0] for w in WALKS])
def test_walk_kinds(name, make, n_fast, n_compiled, checker):
  vol = make()
  shape = tuple(vol.shape[::-1])
  be = ckd.HipBackend(0)
  binary = be.encode(vol, shape)
  assert be.walk_paths() == (n_fast, n_compiled), name
  assert binary == checker.compress(synth.as_numpy_f(vol), parallel=16)
  assert np.array_equal(crackle_amd.decompress(binary), synth.as_numpy_f(vol))


# ---------------------------------------------------------------------------------------------------------------------
# H. caller buffers with guard bands, unaligned views
GUARD = 64 << 10
SENTINEL = 0xA5


class _Ptr:
  """A device address where HipBackend expects a tensor."""
  def __init__(self, ptr, itemsize):
    self.ptr, self.itemsize = ptr, itemsize

  def data_ptr(self):
    return self.ptr

  def element_size(self):
    return self.itemsize


def _guarded(nbytes):
  return torch.full((GUARD + 16 + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)


def _check_guards(buf, start, nbytes, what):
  assert bool((buf[:start] == SENTINEL).all()), ("front guard", what)
  assert bool((buf[start + nbytes:] == SENTINEL).all()), ("back guard", what)


def _bytes_of(arr):
  return torch.from_numpy(np.ascontiguousarray(arr.reshape(-1, order="F")).view(np.uint8)).to(DEV)


# name, shape, dtype, encoder options, env (with its reason), front end
CASES_H = [
  ("records_v2", (100, 300, 3), np.uint32, dict(), {}, "records"),
  ("records_v1", (36, 300, 3), np.uint16, dict(), {}, "records"),
  # the rasterising front end on a small slice: naturally it needs 513 strips (B: raster_16416x513)
  ("raster", (100, 300, 3), np.uint64, dict(), {"CKL_DECODE_RASTER": "1"}, "raster"),
  ("general", (37, 300, 3), np.uint32, dict(), {}, "general"),
  ("pins", (100, 300, 3), np.uint16, dict(allow_pins=True), {}, "records"),
  ("records_u8", (68, 300, 3), np.uint8, dict(markov_model_order=2), {}, "records"),
]


def _offsets(itemsize):
  return sorted({0, 1, 2, 4, 8, 12} if itemsize == 1 else {0, 2, 4, 8, 12, itemsize})


@pytest.mark.parametrize("name,shape,dt,opts,env,front", CASES_H, ids=[c[0] for c in CASES_H])
def test_decode_into_guarded_unaligned_views(name, shape, dt, opts, env, front, checker, monkeypatch):
  arr = synth.as_numpy_f(_dev_volume(shape, dt, cell=(9, 7, 2), seed=shape[0]))
  binary = checker.compress(arr, **opts)
  assert crackle_amd.compress(arr, **opts) == binary
  _set_env(monkeypatch, env)
  p = plan(binary, env=env)
  assert _front(p) == front, p
  if p["strips"]:
    assert shape[1] % p["strip_rows"] != 0, p      # a partial last strip
  want = _bytes_of(arr)
  lab = int(arr[shape[0] // 2, shape[1] // 2, 1])
  want_lab = _bytes_of((arr == lab).astype(np.uint8))
  for off in _offsets(np.dtype(dt).itemsize):
    for label, w in ((None, want), (lab, want_lab)):
      buf = _guarded(w.numel())
      start = GUARD + off
      s = ckd.HipDecodeSession(binary, 0, shape[2], 0)
      try:
        rc = s._L.ckl_decoder_run(s._h, buf.data_ptr() + start, w.numel(), int(label is not None), int(label or 0))
        assert rc == _lib.CKL_OK, _lib.last_error()
        names = [n for n, _ in s.stages()]
      finally:
        s.close()
      torch.cuda.synchronize()
      check_path(names, p, (name, off, label))
      assert torch.equal(buf[start:start + w.numel()], w), (name, off, label)
      _check_guards(buf, start, w.numel(), (name, off, label))
  _set_env(monkeypatch, None)


@pytest.mark.parametrize("sx", [36, 37])
def test_components_into_guarded_unaligned_views(sx):
  """ckl_encoder_components_device: four pixels per store where the rows and the output allow it, one otherwise."""
  shape = (sx, 300, 3)
  vol = _dev_volume(shape, np.uint32, cell=(9, 7, 2), seed=sx)
  be = ckd.HipBackend(0)
  ref = torch.empty((3, 300, sx), dtype=torch.int32, device=DEV)
  nc = be.components_device(vol, shape, 5, ref)
  ref_bytes = ref.reshape(-1).view(torch.uint8).clone()
  n = ref_bytes.numel()
  for off in (1, 2, 4, 8, 12):
    buf = _guarded(n)
    e = be._encoder(shape, 4)
    cnt = np.zeros(3, np.uint32)
    rc = be._L.ckl_encoder_components_device(e, vol.data_ptr(), sx, 300, 3, 5, buf.data_ptr() + GUARD + off, cnt.ctypes.data)
    assert rc == _lib.CKL_OK, _lib.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(cnt, nc)
    assert torch.equal(buf[GUARD + off:GUARD + off + n], ref_bytes), off
    _check_guards(buf, GUARD + off, n, off)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("sx", [64, 68, 37])
def test_encode_unaligned_device_views(sx, dt, checker):
  """The label-plane fast path needs 16-byte aligned rows, the pins' four-column loads 4 labels' worth: an input
  view at other offsets takes the other kernels, with the same bytes."""
  shape = (sx, 40, 4)
  vol = _dev_volume(shape, dt, cell=(9, 7, 2), seed=sx)
  arr = synth.as_numpy_f(vol)
  isz = np.dtype(dt).itemsize
  raw = vol.reshape(-1).view(torch.uint8)
  wants = {kw: checker.compress(arr, **dict(kw)) for kw in ((), (("allow_pins", True),))}
  for off in _offsets(isz):
    buf = _guarded(raw.numel())
    buf[GUARD + off:GUARD + off + raw.numel()] = raw
    ptr = buf.data_ptr() + GUARD + off
    assert (ptr - off) % 256 == 0      # the offset alone decides the view's alignment
    be = ckd.HipBackend(0)
    for kw, want in wants.items():
      assert be.encode(_Ptr(ptr, isz), shape, **dict(kw)) == want, (off, kw)
    _check_guards(buf, GUARD + off, raw.numel(), off)


# ---------------------------------------------------------------------------------------------------------------------
# G. refusals of the slice limit
def _forge_dims(stream, sx, sy):
  b = bytearray(stream)
  b[7:11] = sx.to_bytes(4, "little")
  b[11:15] = sy.to_bytes(4, "little")
  b[28] = ckd._crc8(bytes(b[5:28]))
  return bytes(b)


def test_decoder_refuses_slices_of_2_30_crack_vertices():
  """decoder_build refuses what check_dims would not encode: (sx + 1) (sy + 1) >= 2^30."""
  arr = np.zeros((4, 4, 1), np.uint8)
  arr[1, 1, 0] = 1
  good = crackle_amd.compress(arr)
  h = C.c_void_p()
  L = _lib.lib()
  for sx, sy in ((32767, 32767), (32767, 32768), (65536, 16384), (46336, 46339), (1 << 31, 1)):
    assert (sx + 1) * (sy + 1) >= 1 << 30
    bad = _forge_dims(good, sx, sy)
    assert crackle_amd.header(bad).sx == sx
    assert L.ckl_decoder_create(bad, len(bad), 0, -1, 0, C.byref(h)) == _lib.CKL_ERR_ARG, (sx, sy)
    assert "2^30" in _lib.last_error()
  # one vertex row fewer is not refused for its size (the forged stream's layout is refused instead, if at all)
  for sx, sy in ((32766, 32767), (32767, 32766)):
    assert (sx + 1) * (sy + 1) < 1 << 30
    bad = _forge_dims(good, sx, sy)
    rc = L.ckl_decoder_create(bad, len(bad), 0, -1, 0, C.byref(h))
    if rc == _lib.CKL_OK:
      L.ckl_decoder_destroy(h)
      h = C.c_void_p()
    else:
      assert "2^30" not in _lib.last_error(), (sx, sy)


# ---------------------------------------------------------------------------------------------------------------------
# G. above 2^32 voxels and the largest slice
def test_above_2_32_voxels(checker):
  """2048 x 2048 x 1025 uint8 (4.3 G voxels): the background label alone covers more than 2^32 of them."""
  sx, sy, sz = 2048, 2048, 1025
  vol = torch.zeros((sz, sy, sx), dtype=torch.uint8, device=DEV)
  vol[:, :32, :64] = _dev_volume((64, 32, sz), np.uint8, cell=(8, 8, 4), seed=12)
  vol[:, 1000, 64:1088] = 9
  vol[1024, 1000, 70] = 11
  zeros = int((vol == 0).sum())
  assert zeros > 1 << 32
  be = ckd.HipBackend(0)
  binary = be.encode(vol, (sx, sy, sz))
  assert sum(be.walk_paths()) == sz
  # the z-stack of slabs of <= 512 slices, each encoded alone, is the whole stream; the last slab is the checker's
  slabs = []
  for z0, z1 in ((0, 512), (512, 1024), (1024, 1025)):
    slabs.append(be.encode(vol[z0:z1], (sx, sy, z1 - z0)))
  assert slabs[2] == checker.compress(synth.as_numpy_f(vol[1024:1025]))
  assert crackle_amd.zstack(slabs) == binary
  out = torch.empty_like(vol)
  s = be.open_decoder(binary, 0, sz)
  s.run(out)
  names = [n for n, _ in s.stages()]
  s.close()
  check_path(names, plan(binary), "whole")
  assert torch.equal(out, vol)
  del out
  s = be.open_decoder(binary, 1024, sz)
  last = torch.empty((1, sy, sx), dtype=torch.uint8, device=DEV)
  s.run(last)
  s.close()
  assert torch.equal(last, vol[1024:])
  counts = crackle_amd.voxel_counts(binary)
  assert counts[0] == zeros
  assert counts == {i: int(c) for i, c in enumerate(torch.bincount(vol.reshape(-1), minlength=256).tolist()) if c}


def test_largest_slice():
  """32766 x 32767 x 3 uint8: the largest slice check_dims admits, (sx + 1) (sy + 1) = 2^30 - 2^15 crack vertices;
  3.2 G voxels on the general pipeline (sx % 4 != 0).
  No checker: the reference encodes a few million voxels per second per thread.  The refused side is
  test_decoder_refuses_slices_of_2_30_crack_vertices and tests/test_shape_limits_cpu.py."""
  sx, sy, sz = 32766, 32767, 3
  assert (sx + 1) * (sy + 1) == (1 << 30) - (1 << 15)
  vol = torch.empty((sz, sy, sx), dtype=torch.uint8, device=DEV)
  xs = (torch.arange(sx, device=DEV) // 509).view(1, -1)
  for z in range(sz):
    for y0 in range(0, sy, 4096):
      ys = (torch.arange(y0, min(sy, y0 + 4096), device=DEV) // 331).view(-1, 1)
      vol[z, y0:y0 + ys.shape[0]] = (1 + (ys * 13 + xs * 7 + z) % 250).to(torch.uint8)
  vol[1, sy - 1, sx - 1] = 251
  vol[2, 0, :] = 0
  be = ckd.HipBackend(0)
  binary = be.encode(vol, (sx, sy, sz))
  assert sum(be.walk_paths()) == sz
  p = plan(binary)
  assert not p["strips"] and p["xw"] == 2 and p["yw"] == 2
  out = torch.empty_like(vol)
  s = be.open_decoder(binary, 0, sz)
  s.run(out)
  names = [n for n, _ in s.stages()]
  s.close()
  check_path(names, p, "largest")
  assert torch.equal(out, vol)
  del out
  s = be.open_decoder(binary, 2, 3)
  last = torch.empty((1, sy, sx), dtype=torch.uint8, device=DEV)
  s.run(last)
  s.close()
  assert torch.equal(last, vol[2:])
  counts = crackle_amd.voxel_counts(binary)
  assert counts == {i: int(c) for i, c in enumerate(torch.bincount(vol.reshape(-1), minlength=256).tolist()) if c}
