"""GPU tests of the encoder's label stage on the strip kernels (crackle_amd/csrc/ckl_strips.hpp: strip_ccl_body and
slice_resolve_body in their encoder modes; ckl_encode_labels.hip: k_strip_ccl_enc, k_gather_slots, flat_enqueue /
flat_collect) and of its hand-over to the run pipeline of ckl_runs.hpp.

The check throughout: crackle_amd.compress(arr, ...) equals the checker's compress byte for byte, once on the default
path and once with the run pipeline forced (CKL_ENC_LABEL_RUNS), and the stream decodes back to arr (the decoder
verifies the per-slice crcs of the component images again).  Every case names the point where the path can go wrong."""
import numpy as np
import pytest

import crackle_amd
from crackle_amd import synth

pytestmark = pytest.mark.gpu

KSTRIP_WORDS = 1024      # ckl_strips.hpp kStripWords: plane words per strip


def _vol(shape, dt, seed, cell=(16, 16, 4), **kw):
  return synth.as_numpy_f(synth.voronoi_labels(shape, dt, seed=seed, cell=cell, **kw))


def _check(arr, checker, monkeypatch, capfd=None, marks=(), **kw):
  """marks: what the host timer's line of the default encode (CKL_PROFILE, on stderr) must name, so that a case shows
  the path it is about: f:enqueue_strips (the strip kernels were launched), f:resolve_retry (the resolve ran again
  with a CU's LDS), f:wait_strips / f:wait_runs (where the collected results came from)."""
  want = checker.compress(arr, **kw)
  monkeypatch.delenv("CKL_ENC_LABEL_RUNS", raising=False)
  if capfd is not None:
    monkeypatch.setenv("CKL_PROFILE", "1")
    capfd.readouterr()
  got = crackle_amd.compress(arr, **kw)
  if capfd is not None:
    monkeypatch.delenv("CKL_PROFILE", raising=False)
    lines = [l for l in capfd.readouterr().err.splitlines() if l.startswith("[ckl encode host ms]")]
    assert lines, "no host timer line on stderr"
    seen = sorted(w.split("=")[0] for w in lines[-1].split() if w.startswith("f:"))
    for m in marks:
      assert m in seen, f"{m} not among {seen} {arr.shape}"
    assert ("f:wait_strips" in seen) != ("f:wait_runs" in seen)
  assert got == want, f"default label path {arr.shape} {arr.dtype} {kw}"
  monkeypatch.setenv("CKL_ENC_LABEL_RUNS", "1")
  assert crackle_amd.compress(arr, **kw) == want, f"run pipeline forced {arr.shape} {arr.dtype} {kw}"
  monkeypatch.delenv("CKL_ENC_LABEL_RUNS", raising=False)
  back = crackle_amd.decompress(got)
  assert back.dtype == arr.dtype and np.array_equal(back, arr)
  return got


SHAPES = [
  ((4, 4, 2), np.uint8, (2, 2, 1)),             # one strip, one word
  ((33, 1, 1), np.uint32, (4, 1, 1)),           # a ragged last word, a single-row strip
  ((1, 40, 2), np.uint32, (1, 4, 1)),           # single-column strips: every run is one pixel
  ((36, 300, 3), np.uint64, (8, 8, 4)),         # two words per row, 8-byte labels above 2^40
  ((320, 288, 5), np.uint32, (16, 16, 4)),      # several strips
  ((2048, 40, 2), np.uint32, (32, 32, 8)),      # 64 words per row
]


@pytest.mark.parametrize("shape,dt,cell", SHAPES)
def test_shapes(shape, dt, cell, checker, monkeypatch, capfd):
  arr = _vol(shape, dt, seed=41, cell=cell, offset=(1 << 40) if dt == np.uint64 else 0)
  if dt == np.uint64:
    assert int(arr.min()) >= (1 << 40)
  _check(arr, checker, monkeypatch, capfd, ("f:enqueue_strips", "f:wait_strips"))
  _check(arr, checker, monkeypatch, markov_model_order=3)


def test_c_order_and_single_slice(checker, monkeypatch):
  arr = np.ascontiguousarray(_vol((96, 80, 6), np.uint32, seed=42))
  assert arr.flags.c_contiguous and not arr.flags.f_contiguous
  _check(arr, checker, monkeypatch)
  _check(_vol((320, 288, 1), np.uint16, seed=43), checker, monkeypatch)


# ---- seams and first pixels: rows of 64 pixels are two plane words, so a strip has at most 512 rows; the patterns
# below cross a seam wherever the encoder puts it (it sizes the strips from the run density)
SEAM_ROWS = KSTRIP_WORDS // 2
SEAM_SHAPE = (64, 3 * SEAM_ROWS + 1, 2)


def _seam_volume(kind):
  sx, sy, sz = SEAM_SHAPE
  a = np.zeros(SEAM_SHAPE, dtype=np.uint32, order="F")
  if kind == "stripes":
    # vertical stripes crossing every seam, another set of labels in the second slice
    for z in range(sz):
      a[:, :, z] = (np.arange(sx, dtype=np.uint32)[:, None] // 5) * 3 + 7 + 100 * z
  elif kind == "u":
    # a "U": two arms that meet only in the last row, so only in the last strip; its id and label come from
    # the left arm's first pixel.  The background is split by it into an inside and an outside part.
    a[:] = 5
    a[10:13, :, :] = 9
    a[40:43, :, :] = 9
    a[10:43, sy - 1, :] = 9
    a[:, :, 1] += 11
  elif kind == "ring":
    a[:] = 3
    a[8:56, 2:sy - 2, :] = 4
    a[12:52, 6:sy - 6, :] = 3      # the inside has the outside's label but is another component
  elif kind == "comb":
    # teeth that hang from a bar in the last row: every tooth is its own strip component until the last strip
    a[:] = 2
    a[1::4, :, :] = 6
    a[:, sy - 1, :] = 6
  elif kind == "rows":
    # two labels alternating row by row: every seam separates, nothing unites
    a[:, 0::2, :] = 21
    a[:, 1::2, :] = 22
  return a


@pytest.mark.parametrize("kind", ["stripes", "u", "ring", "comb", "rows"])
def test_seams_and_first_pixels(kind, checker, monkeypatch):
  _check(_seam_volume(kind), checker, monkeypatch)


def _blocks(shape, bx, by, dt):
  """Blocks of bx x by pixels with pairwise different labels within a slice."""
  sx, sy, sz = shape
  x = np.arange(sx)[:, None, None] // bx
  y = np.arange(sy)[None, :, None] // by
  z = np.arange(sz)[None, None, :]
  return np.asfortranarray((1 + x + (sx // bx) * y + 17 * z).astype(dt))


@pytest.mark.parametrize("bx,by", [(8, 8), (64, 32)])
def test_narrow_and_wide_strip_component_ids(bx, by, checker, monkeypatch, capfd):
  # 32 words per row: strips of at most 32 rows.  8 x 8 blocks: 128 components per block row, more than 256 per
  # strip (16-bit ids of the strip components); 64 x 32 blocks: 16 per block row, at most 256 (8-bit ids)
  arr = _blocks((1024, 96, 2), bx, by, np.uint16)
  assert len(np.unique(arr[:, :, 0])) == (1024 // bx) * (96 // by)
  _check(arr, checker, monkeypatch, capfd, ("f:enqueue_strips", "f:wait_strips"))


def test_resolve_again_with_a_whole_cu(checker, monkeypatch, capfd):
  # 21 760 single pixels with pairwise different labels in a background, 1024 x 512: more strip components per slice
  # than the resolve's table beside the walk holds (9152), fewer than a CU's LDS does; the pixels touch nothing, so the
  # crack graph has no branching nodes and the label stage starts with the walk
  a = np.full((1024, 512, 2), 7, dtype=np.uint32, order="F")
  xs, ys = np.arange(1, 1024, 4), np.arange(1, 512, 6)
  ids = 100 + np.arange(xs.size * ys.size, dtype=np.uint32).reshape(xs.size, ys.size)
  for z in range(2):
    a[np.ix_(xs, ys, [z])] = (ids + 50000 * z)[:, :, None]
  assert xs.size * ys.size + 1 > 9152
  _check(a, checker, monkeypatch, capfd, ("f:enqueue_strips", "f:resolve_retry", "f:wait_strips"))


def test_hand_over_noise(checker, monkeypatch, capfd):
  _check(synth.random_labels((256, 256, 4), np.uint32, seed=5, high=2000), checker, monkeypatch, capfd, ("f:wait_runs",))
  _check(synth.random_labels((512, 64, 3), np.uint8, seed=6, high=2), checker, monkeypatch, capfd, ("f:wait_runs",), markov_model_order=2)


def test_hand_over_one_noise_slice(checker, monkeypatch, capfd):
  arr = _vol((256, 192, 5), np.uint32, seed=44).copy(order="F")
  arr[:, :, 2] = synth.random_labels((256, 192, 1), np.uint32, seed=7, high=2000)[:, :, 0]
  _check(arr, checker, monkeypatch, capfd, ("f:wait_runs",))


@pytest.mark.parametrize("switch,value", [("CKL_ENC_RESOLVE_CAP", "7"), ("CKL_ENC_STRIP_CAP", "64")])
def test_hand_over_forced_by_the_caps(switch, value, checker, monkeypatch, capfd):
  arr = _vol((320, 288, 5), np.uint32, seed=32)
  _check(arr, checker, monkeypatch, capfd, ("f:enqueue_strips", "f:wait_strips"))
  monkeypatch.setenv(switch, value)
  # the strips were launched, a table overflowed, the run pipeline redid the volume
  _check(arr, checker, monkeypatch, capfd, ("f:enqueue_strips", "f:enqueue_runs", "f:wait_runs"))


@pytest.mark.parametrize("resident", [False, True])
def test_session_reuse(resident, checker):
  """One encoder session: smooth, noise (handed over to the run pipeline), smooth again."""
  import torch
  from crackle_amd import distributed as ckd
  dev = torch.device("cuda", 0)
  shape_a, shape_b = (320, 288, 5), (256, 256, 4)
  smooth = synth.voronoi_labels(shape_a, np.uint32, seed=45, cell=(16, 16, 4), device=dev)
  noise = synth.random_labels_device(shape_b, np.uint32, seed=8, high=2000, device=dev)
  be = ckd.HipBackend(0)
  if resident:
    # as bench.py sets them: the stream stays in HBM, the host copy of the codes runs in the background
    be.keep_device_stream(shape_a, 4, True)
    be.async_host_copy(shape_a, 4, True)
  session = be._encoder(shape_a, 4).value

  def encode(vol, shape):
    # HipBackend opens a new session for another shape; the library's session takes any shape of its dtype
    # (ckl_encoder_run), and one session is what this test is about
    be._enc_key = (tuple(shape), 4)
    out = bytes(be.encode(vol, shape, False, True, 0, None))
    assert be._enc.value == session
    return out

  first = encode(smooth, shape_a)
  middle = encode(noise, shape_b)
  third = encode(smooth, shape_a)
  assert first == third
  assert first == checker.compress(synth.as_numpy_f(smooth))
  assert middle == checker.compress(synth.as_numpy_f(noise))
  assert np.array_equal(crackle_amd.decompress(third), synth.as_numpy_f(smooth))


def test_pins_and_components_keep_the_run_pipeline(checker, monkeypatch, capfd):
  import torch
  from crackle_amd import distributed as ckd
  shape = (256, 192, 6)
  arr = _vol(shape, np.uint32, seed=46)
  got = _check(arr, checker, monkeypatch, capfd, ("f:enqueue_runs", "f:wait_runs"), allow_pins=True)
  # 3-D components of the stream: the same bytes whichever label path encoded it
  want_cc = crackle_amd.connected_components(checker.compress(arr))
  assert crackle_amd.connected_components(_check(arr, checker, monkeypatch)) == want_cc
  assert crackle_amd.header(got).sz == shape[2]
  # the encoder's own 2-D components (ckl_encoder_components): ids in raster order of first pixels, one label each
  vol = synth.voronoi_labels(shape, np.uint32, seed=46, cell=(16, 16, 4), device=torch.device("cuda", 0))
  cc = np.zeros(shape[0] * shape[1] * shape[2], dtype=np.uint32)
  nc = np.zeros(shape[2], dtype=np.uint32)
  ckd.HipBackend(0).components(vol, shape, 0, cc, nc)
  flat = arr.reshape(-1, order="F")
  ids, first_at = np.unique(cc, return_index=True)
  assert len(ids) == int(nc.sum()) and np.array_equal(ids, np.arange(len(ids), dtype=np.uint32))
  assert np.all(np.diff(first_at) > 0)
  assert np.array_equal(flat[first_at][cc], flat)
