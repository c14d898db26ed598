"""GPU tests of cutout (crackle_amd/csrc/ckl_operations.hip: k_paint_window behind ckl_decoder_cutout and
ckl_cutout; crackle_amd/array.py: cutout, CrackleArray).  Every expected value is vol[expr] of the
numpy array the stream was made from.  Boxes are read through a session (ckl_decoder_cutout into one
device buffer per session, every box at the byte offset where the one before ended, so that the
output's base is aligned to nothing but the element) and through cutout() / CrackleArray[...]."""
import ctypes as C
import functools
import itertools
import os

import numpy as np
import pytest

import contacts_numpy as cn
import crackle_amd
import golden_cases
from crackle_amd import _lib, synth
from util import golden

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
S = np.s_

# k_paint_window's constants (ckl_operations.hip), restated: a workgroup takes whole window rows of up
# to kWinTile pixels, at most kWinRows of them, and stages up to kWinStage run labels
K_WIN_TILE, K_WIN_ROWS, K_WIN_STAGE = 4096, 64, 1536


@functools.lru_cache(maxsize=None)
def _voronoi(shape, dtype, order):
  """The three slice geometries of tests/test_gpu_contacts.py: (volume, its stream)."""
  vol = synth.as_numpy_f(synth.voronoi_labels(shape, dtype, seed=31, cell=(8, 8, 3)))
  vol = np.ascontiguousarray(vol) if order == "C" else np.asfortranarray(vol)
  return vol, bytes(crackle_amd.compress(vol))


GEOMETRIES = [((97, 61, 7), np.uint16, "F"), ((128, 64, 9), np.uint32, "F"), ((96, 80, 6), np.uint8, "C")]
GEOMETRY_IDS = ["97x61x7-u16-F", "128x64x9-u32-F", "96x80x6-u8-C"]


class Session:
  """ckl_decoder_create over [z0, z1) and ckl_decoder_cutout into torch device buffers."""

  def __init__(self, binary, z0=0, z1=-1):
    self.L = _lib.lib()
    self.h = C.c_void_p()
    self.binary = binary
    rc = self.L.ckl_decoder_create(binary, len(binary), z0, z1, 0, C.byref(self.h))
    assert rc == _lib.CKL_OK, _lib.last_error()

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.L.ckl_decoder_destroy(self.h)

  def cutout(self, box, ptr, capacity, label=None):
    x0, x1, y0, y1 = box
    return self.L.ckl_decoder_cutout(self.h, x0, x1, y0, y1, ptr, capacity, int(label is not None), int(label or 0))


def _boxes_through_a_session(binary, vol, z0, z1, boxes, label=None):
  """Every box of slices [z0, z1) against vol; the boxes share one device buffer, end to end."""
  import torch
  head = crackle_amd.header(binary)
  order = "F" if head.fortran_order else "C"
  width = 1 if label is not None else vol.dtype.itemsize
  sizes = [(x1 - x0) * (y1 - y0) * (z1 - z0) * width for x0, x1, y0, y1 in boxes]
  buf = torch.full((sum(sizes) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
  with Session(binary, z0, z1) as s:
    at = 0
    for box, n in zip(boxes, sizes):
      rc = s.cutout(box, buf.data_ptr() + at, n, label)
      assert rc == _lib.CKL_OK, (box, _lib.last_error())
      at += n
  host = buf.cpu().numpy()
  assert (host[at:] == 0xA5).all(), "bytes behind the last box were written"
  want_all = (vol == label) if label is not None else vol
  at = 0
  for (x0, x1, y0, y1), n in zip(boxes, sizes):
    got = host[at:at + n].view(bool if label is not None else vol.dtype).reshape((x1 - x0, y1 - y0, z1 - z0), order=order)
    want = want_all[x0:x1, y0:y1, z0:z1]
    assert np.array_equal(got, want), ((x0, x1, y0, y1, z0, z1), np.argwhere(got != want)[:4])
    at += n


@pytest.mark.parametrize("shape,dtype,order", GEOMETRIES, ids=GEOMETRY_IDS)
def test_word_and_edge_arithmetic(shape, dtype, order):
  """x-bounds on, before and behind the 32-pixel word boundaries and the slice's edges; z-ranges that do
  not start at 0, where comp_off, rbase and the planes are indexed by the session's slice, not by z."""
  vol, binary = _voronoi(shape, dtype, order)
  sx, sy, sz = shape
  xs = sorted({0, 1, 31, 32, 33, 63, 64, sx - 1, sx})
  ys = [(0, 1), (sy - 1, sy), (3, sy - 2), (0, sy)]
  boxes = [(x0, x1, y0, y1) for x0, x1 in itertools.combinations(xs, 2) for y0, y1 in ys]
  assert len(boxes) == 36 * 4
  for z0, z1 in ((0, sz), (2, 3), (sz - 1, sz)):
    _boxes_through_a_session(binary, vol, z0, z1, boxes)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.uint64], ids=lambda d: np.dtype(d).name)
def test_every_width_with_odd_boxes(dtype):
  """Boxes 5 and 1 pixels wide at x0 = 3: no row of the output starts where the one before did modulo
  16 bytes, so no vector store may assume its alignment."""
  vol = synth.as_numpy_f(synth.voronoi_labels((97, 61, 5), dtype, seed=33, cell=(8, 8, 3), offset=(1 << 40) if dtype == np.uint64 else 0))
  binary = bytes(crackle_amd.compress(vol))
  _boxes_through_a_session(binary, vol, 0, 5, [(3, 8, 0, 61), (3, 4, 0, 61), (3, 8, 7, 18), (3, 4, 60, 61), (90, 97, 1, 60)])
  for expr in (S[3:8], S[3:4], S[3:8, 5:50, 1:4], S[3, :, 2]):
    got = crackle_amd.cutout(binary, expr)
    assert got.dtype == vol.dtype and np.array_equal(got, vol[expr]), expr


def test_signed_stream_keeps_its_negative_labels(checker):
  lab, kw = cn.signed_volumes()["signed_int16_p0"]
  binary = checker.compress(lab, **kw)
  assert (lab < 0).any()
  for expr in (S[3:30, 2:33, 1:5], S[5, ::2], S[..., -1], S[:, :, :]):
    got = crackle_amd.CrackleArray(binary)[expr]
    assert got.dtype == np.int16 and np.array_equal(got, lab[expr]), expr
  assert (crackle_amd.cutout(binary, S[3:30, 2:33, 1:5]) < 0).any()
  arr = crackle_amd.CrackleArray(binary)
  assert arr.dtype == np.int16 and arr.min() == int(lab.min()) < 0 and arr.max() == int(lab.max())


def test_label_gives_a_bool_box():
  vol, binary = _voronoi(*GEOMETRIES[0])
  present = [int(vol[40, 30, 3]), int(vol[96, 0, 0])]
  assert 0 not in np.unique(vol)      # voronoi labels start at 1: the background is absent here
  for label in present:
    for expr in (S[33:70, 5:61, 1:6], S[:, 29:31], S[::3, 4, ::2]):
      got = crackle_amd.cutout(binary, expr, label=label)
      assert got.dtype == bool and np.array_equal(got, (vol == label)[expr]), (label, expr)
    _boxes_through_a_session(binary, vol, 2, 6, [(31, 65, 3, 59), (1, 97, 0, 61)], label=label)
  # the background where it is present: a volume with a block of zeros
  vol0 = np.asfortranarray(vol.copy())
  vol0[20:50, 10:40, 2:5] = 0
  binary0 = bytes(crackle_amd.compress(vol0))
  for expr in (S[10:60, 5:45, 1:6], S[25, :, :], S[...]):
    got = crackle_amd.cutout(binary0, expr, label=0)
    assert got.dtype == bool and got.any() and np.array_equal(got, (vol0 == 0)[expr]), expr


def test_pin_labels_markov_and_version_0():
  cases = golden_cases.small_cases()
  vol = cases["c0_voronoi_u8_pins_m5"][0]
  binary = golden()["c0_voronoi_u8_pins_m5"]
  exprs = (S[1:63, 1:63, 1:15], S[31:34, :, 5:6], S[:, 63, :], S[7:50:3, 33:, 9:], S[0:33, 0:64, 4:16])
  for expr in exprs:
    assert np.array_equal(crackle_amd.cutout(binary, expr), vol[expr]), expr
  _boxes_through_a_session(binary, vol, 5, 11, [(1, 64, 0, 64), (30, 35, 10, 11)], label=int(vol[32, 10, 7]))
  with np.load(os.path.join(HERE, "golden", "v0.npz")) as z:
    names = [k for k in z.files if "." not in k]
    v0 = {k: z[k].tobytes() for k in names}
  for name in ("c0_voronoi_u8", "c0_voronoi_u8_c", "rand_17x13x5_uint64_F_m3_p1"):      # flat F, flat C, pins + markov
    vol = cases[name][0]
    assert crackle_amd.header(v0[name]).format_version == 0
    sx, sy, sz = vol.shape
    for expr in (S[1:sx - 1, 1:sy - 1, :], S[sx // 2, :, sz - 1], S[::2, 3:, ...], S[1:2, 2:9, 1:3]):
      assert np.array_equal(crackle_amd.cutout(v0[name], expr), vol[expr]), (name, expr)


def _runs_of_rows(vol, z, y0, y1, x0, x1):
  """Runs that window rows y0 .. y1 - 1 of slice z cross: a run ends where the label changes along x."""
  rows = vol[x0:x1, y0:y1, z]
  return int((rows[1:] != rows[:-1]).sum()) + (y1 - y0)


def test_staging_and_its_overflow():
  """Binary noise has a run per pixel or two: the 16 rows of a full-width tile cross more runs than the
  stage holds, and the kernel looks labels up in HBM.  A voronoi box stays below and is staged."""
  noise = synth.random_labels((256, 64, 2), np.uint8, seed=13, high=2)
  binary = bytes(crackle_amd.compress(noise))
  box = (1, 256, 0, 64)      # not the whole plane: ckl_cutout keeps it on the window kernel
  rows = min(K_WIN_ROWS, K_WIN_TILE // (box[1] - box[0]))
  assert rows == 16
  for z in range(2):
    for y in range(0, 64, rows):
      assert _runs_of_rows(noise, z, y, y + rows, box[0], box[1]) > K_WIN_STAGE
  _boxes_through_a_session(binary, noise, 0, 2, [box, (0, 255, 1, 63), (0, 256, 0, 64)])
  assert np.array_equal(crackle_amd.cutout(binary, S[1:]), noise[1:])
  for label in (0, 1):
    assert np.array_equal(crackle_amd.cutout(binary, S[1:, :63], label=label), (noise == label)[1:, :63])
  vol, vbinary = _voronoi(*GEOMETRIES[1])
  vbox = (1, 128, 0, 64)
  vrows = min(K_WIN_ROWS, K_WIN_TILE // 127)
  for z in range(vol.shape[2]):
    for y in range(0, 64, vrows):
      assert _runs_of_rows(vol, z, y, min(64, y + vrows), vbox[0], vbox[1]) <= K_WIN_STAGE
  _boxes_through_a_session(vbinary, vol, 0, vol.shape[2], [vbox])


def _random_expression(rng, shape):
  parts = []
  for dim in shape:
    kind = rng.integers(0, 10)
    if kind < 2:
      parts.append(int(rng.integers(-dim, dim)))
    elif kind < 3:
      parts.append(slice(None))
    else:
      a, b = sorted(int(v) for v in rng.integers(0, dim + 1, 2))
      if rng.integers(0, 4) == 0:
        a = a - dim if a < dim else a      # the same bound, counted from the end
      if rng.integers(0, 4) == 0 and b < dim:
        b = b - dim
      step = None if rng.integers(0, 2) else int(rng.integers(1, 5))
      parts.append(slice(a if rng.integers(0, 8) else None, b if rng.integers(0, 8) else None, step))
  cut = int(rng.integers(0, 8))
  if cut == 0:
    parts = parts[:2]
  elif cut == 1:
    parts = parts[:1] + [Ellipsis] + parts[2:]
  elif cut == 2:
    parts = [Ellipsis] + parts[1:] if rng.integers(0, 2) else [Ellipsis] + parts[2:]
  return tuple(parts)


@pytest.mark.parametrize("shape,dtype,order", GEOMETRIES, ids=GEOMETRY_IDS)
def test_random_index_expressions(shape, dtype, order):
  vol, binary = _voronoi(shape, dtype, order)
  arr = crackle_amd.CrackleArray(binary)
  rng = np.random.default_rng(20 + shape[0])
  kinds = set()
  for _ in range(150):
    expr = _random_expression(rng, shape)
    want = vol[expr]
    got = arr[expr]
    assert got.shape == want.shape and got.dtype == vol.dtype and np.array_equal(got, want), expr
    kinds.update(type(p).__name__ for p in expr)
    kinds.update("step" for p in expr if isinstance(p, slice) and p.step not in (None, 1))
    kinds.update("negative" for p in expr if isinstance(p, int) and p < 0)
  assert kinds >= {"int", "slice", "ellipsis", "step", "negative"}, kinds


def test_device_output_and_argument_errors():
  import torch
  vol, binary = _voronoi(*GEOMETRIES[0])
  sx, sy, sz = vol.shape
  L = _lib.lib()
  with Session(binary, 1, 6) as s:
    a = torch.empty((40 * 50 * 5,), dtype=torch.int16, device="cuda")
    b = torch.empty((97 * 2 * 5,), dtype=torch.int16, device="cuda")
    assert s.cutout((10, 50, 5, 55), a.data_ptr(), a.numel() * 2) == _lib.CKL_OK, _lib.last_error()
    assert s.cutout((0, 97, 59, 61), b.data_ptr(), b.numel() * 2) == _lib.CKL_OK, _lib.last_error()
    assert np.array_equal(a.cpu().numpy().view(np.uint16).reshape((40, 50, 5), order="F"), vol[10:50, 5:55, 1:6])
    assert np.array_equal(b.cpu().numpy().view(np.uint16).reshape((97, 2, 5), order="F"), vol[:, 59:61, 1:6])
    # the kernel is the last stage of the session's timing table
    names = []
    for i in range(32):
      name, ms = C.c_char_p(), C.c_float()
      if L.ckl_decoder_stage_timing(s.h, i, C.byref(name), C.byref(ms)) != _lib.CKL_OK:
        break
      names.append(name.value.decode())
    assert names[-1] == "k_paint_window" and names.count("k_paint_window") == 1, names
    assert s.cutout((10, 50, 5, 55), a.data_ptr(), a.numel() * 2 - 1) == _lib.CKL_ERR_ARG
    assert "too small" in _lib.last_error()
    for box, axis in (((0, sx + 1, 0, sy), "x range"), ((5, 4, 0, sy), "x range"), ((-1, 4, 0, sy), "x range"), ((0, sx, 3, sy + 1), "y range"), ((0, sx, 9, 8), "y range")):
      assert s.cutout(box, a.data_ptr(), a.numel() * 2) == _lib.CKL_ERR_ARG, box
      assert axis in _lib.last_error(), (box, _lib.last_error())
    assert s.cutout((7, 7, 0, sy), None, 0) == _lib.CKL_OK      # an empty box writes nothing
  out = np.empty((4 * 4 * 2,), np.uint16)

  def one_shot(x0, x1, y0, y1, z0, z1, cap=out.nbytes):
    return L.ckl_cutout(binary, len(binary), out.ctypes.data, cap, _lib.MEM_HOST, x0, x1, y0, y1, z0, z1, 0, 0, 0)

  assert one_shot(0, 4, 0, 4, 5, 7) == _lib.CKL_OK and np.array_equal(out.reshape((4, 4, 2), order="F"), vol[:4, :4, 5:7])
  assert one_shot(0, 4, 0, 4, 5, sz + 1) == _lib.CKL_ERR_ARG and "z range" in _lib.last_error()
  assert one_shot(0, 4, 0, 4, 3, 2) == _lib.CKL_ERR_ARG and "z range" in _lib.last_error()
  assert one_shot(0, sx + 1, 0, 4, 0, 1) == _lib.CKL_ERR_ARG and "x range" in _lib.last_error()
  assert one_shot(0, 4, 0, 4, 5, 7, cap=out.nbytes - 1) == _lib.CKL_ERR_ARG and "too small" in _lib.last_error()
  dev = torch.empty((4 * 4 * 2,), dtype=torch.int16, device="cuda")
  rc = L.ckl_cutout(binary, len(binary), dev.data_ptr(), 64, _lib.MEM_DEVICE, 93, 97, 57, 61, 0, 2, 0, 0, 0)
  assert rc == _lib.CKL_OK and np.array_equal(dev.cpu().numpy().view(np.uint16).reshape((4, 4, 2), order="F"), vol[93:, 57:, :2])


@pytest.mark.parametrize("shape,dtype,order", GEOMETRIES, ids=GEOMETRY_IDS)
def test_full_plane_is_the_decode(shape, dtype, order):
  vol, binary = _voronoi(shape, dtype, order)
  sx, sy, sz = shape
  want = crackle_amd.decompress_range(binary, 1, sz - 1)
  out = np.empty((sx * sy * (sz - 2),), dtype)
  rc = _lib.lib().ckl_cutout(binary, len(binary), out.ctypes.data, out.nbytes, _lib.MEM_HOST, 0, sx, 0, sy, 1, sz - 1, 0, 0, 0)
  assert rc == _lib.CKL_OK, _lib.last_error()
  assert out.tobytes() == want.tobytes(order="A")
  assert np.array_equal(want, vol[:, :, 1:sz - 1])


def test_a_damaged_slice_raises_as_for_a_decode():
  """One byte in the middle of slice 3's crack code is flipped.  A cutout whose z-range holds the slice
  raises what the decode of that range raises, wherever the box lies; one that leaves it out reads clean."""
  vol = golden_cases.small_cases()["c0_voronoi_u8"][0]
  good = golden()["c0_voronoi_u8"]
  head = crackle_amd.header(good)
  zidx = np.frombuffer(good, dtype="<u4", offset=head.header_bytes, count=head.sz).astype(np.int64)
  start = head.header_bytes + head.grid_index_bytes + head.num_label_bytes + head.markov_model_bytes + int(zidx[:3].sum())
  bad = bytearray(good)
  bad[start + int(zidx[3]) // 2] ^= 0x04
  bad = bytes(bad)
  assert crackle_amd.check(bad)["z"] == [3]
  with pytest.raises(RuntimeError) as info:
    crackle_amd.decompress(bad)
  message = str(info.value)
  assert "z=3" in message
  damaged = np.argwhere(crackle_amd.decompress(good)[:, :, 3] != vol[:, :, 3])
  assert damaged.size == 0      # (the good stream decodes to the volume)
  for expr in (S[0:4, 0:4, 3:4], S[60:64, 60:64, 0:8], S[:, 1:, 3], S[5, 5, :]):
    with pytest.raises(RuntimeError) as info:
      crackle_amd.cutout(bad, expr)
    assert type(info.value) is RuntimeError and str(info.value) == message, expr
  for expr in (S[:, 1:, :3], S[1:30, 2:60, 4:], S[7, 7, 2], S[..., 4]):
    assert np.array_equal(crackle_amd.cutout(bad, expr), vol[expr]), expr
