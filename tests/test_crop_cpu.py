"""crop, crop_boxes and chunks without a GPU: the restatement (tests/crop_numpy.py) pinned by literal loops; what the volumes
and boxes of tests/crop_volumes.py hold (none of them is vacuous); chunk_boxes against its restatement; the public
surface, and everything the host answers without a device (through Python and through the C entries)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import crackle_amd
import crop_numpy
import crop_volumes as volumes
from crackle_amd import _lib, array
from crackle_amd import crop, crop_boxes, chunks, chunk_boxes      # (the feature under test: without it nothing here runs)
from recompress_volumes import as_signed, permissible
from util import golden

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_restatement_is_the_literal_triple_loop():
  rng = np.random.default_rng(5)
  vol = np.asfortranarray(rng.integers(0, 9, (9, 7, 5)).astype(np.uint16))
  for box in ((0, 9, 0, 7, 0, 5), (2, 7, 1, 6, 3, 4), (8, 9, 0, 1, 4, 5), (3, 3, 0, 7, 0, 5)):
    x0, x1, y0, y1, z0, z1 = box
    want = np.zeros((x1 - x0, y1 - y0, z1 - z0), np.uint16)
    for x in range(x0, x1):
      for y in range(y0, y1):
        for z in range(z0, z1):
          want[x - x0, y - y0, z - z0] = vol[x, y, z]
    for v in (vol, np.ascontiguousarray(vol)):
      out = crop_numpy.crop(v, box)
      assert out.dtype == vol.dtype and out.shape == want.shape and np.array_equal(out, want)
      assert out.base is None or not np.shares_memory(out, v)
      if out.size > 1 and min(out.shape) > 1:
        assert out.flags.f_contiguous == v.flags.f_contiguous and out.flags.c_contiguous == v.flags.c_contiguous
    assert crop_numpy.in_bounds(box, vol.shape) and np.array_equal(vol[crop_numpy.slices(box)], want)
  assert not crop_numpy.in_bounds((0, 10, 0, 7, 0, 5), vol.shape) and not crop_numpy.in_bounds((3, 2, 0, 7, 0, 5), vol.shape)


def test_restated_runs():
  row = np.array([1, 1, 2, 2, 2, 1, 0], np.uint8).reshape((7, 1, 1), order="F")
  assert crop_numpy.x_runs(row) == 4
  assert crop_numpy.x_runs(np.repeat(np.repeat(row, 3, axis=1), 2, axis=2)) == 24
  assert crop_numpy.x_runs(np.zeros((5, 4, 3), np.uint8)) == 12


# ---- chunk_boxes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,size", [
  ((64, 64, 8), (32, 32, 4)), ((70, 50, 13), (32, 32, 4)), ((70, 50, 13), (70, 50, 13)), ((70, 50, 13), (100, 100, 100)),
  ((5, 4, 3), (1, 1, 1)), ((5, 4, 3), (2, 3, 2)), ((33, 1, 1), (32, 1, 1)), ((7, 0, 3), (2, 2, 2)),
], ids=lambda v: "x".join(map(str, v)))
def test_chunk_boxes(shape, size):
  boxes = chunk_boxes(shape, size)
  assert boxes == crop_numpy.chunk_boxes(shape, size)
  seen = np.zeros(shape, np.int32)
  for b in boxes:
    assert crop_numpy.in_bounds(b, shape) and all(0 < b[2 * k + 1] - b[2 * k] <= size[k] for k in range(3))
    assert all(b[2 * k] % size[k] == 0 for k in range(3))
    seen[crop_numpy.slices(b)] += 1
  assert (seen == 1).all()      # every voxel exactly once
  assert len(boxes) == (0 if 0 in shape else int(np.prod([-(-s // c) for s, c in zip(shape, size)])))
  assert len({b[k] for b in boxes for k in ()} | {(b[1] - b[0], b[3] - b[2], b[5] - b[4]) for b in boxes}) <= 8      # at most eight shapes
  origins = [(b[0], b[2], b[4]) for b in boxes]
  assert origins == sorted(origins, key=lambda o: (o[2], o[1], o[0]))      # x fastest


def test_chunk_sizes_below_one_are_refused():
  binary = golden()["c0_voronoi_u8"]
  for size in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (4, 4), (4, 4, 4, 4), 4, (1.5, 2, 2)):
    with pytest.raises(ValueError, match="chunk_size"):
      chunk_boxes((8, 8, 8), size)
    with pytest.raises(ValueError, match="chunk_size"):
      chunks(binary, size)
    with pytest.raises(ValueError, match="chunk_size"):
      crackle_amd.CrackleArray(binary).chunks(size)


# ---- what the GPU tests rely on ----------------------------------------------------------------------------------------
def _changes(row):
  return tuple((np.flatnonzero(row[1:] != row[:-1]) + 1).tolist())


@pytest.mark.parametrize("sx", volumes.EDGE_SX)
def test_edge_volumes_and_boxes_hold_what_they_claim(sx):
  vol = volumes.edges(sx)
  assert vol.shape == (sx, 3, 3) and vol.dtype == np.uint8
  cols = volumes.edge_cols(sx)
  assert cols == tuple(c for c in (1, 31, 32, 33, 62, 63, 64, 65, 95, 96) if c < sx) and len(cols) >= 3
  for y in range(3):
    for z in range(3):
      assert _changes(vol[:, y, z]) == cols
  assert not np.array_equal(vol[:, 0, 0], vol[:, 1, 0]) and not np.array_equal(vol[:, :, 0], vol[:, :, 1])
  boxes = volumes.edge_boxes(sx)
  assert len(boxes) == len(set(boxes)) and all(crop_numpy.in_bounds(b, vol.shape) for b in boxes)
  fits = [(x0, w) for x0 in (0, 1, 31, 32, 33, 63, 64) for w in (1, 2, 31, 32, 33, 64, 65) if x0 + w <= sx]
  assert {(b[0], b[1] - b[0]) for b in boxes} == set(fits) and len(boxes) == 4 * len(fits)
  assert {(b[2], b[4]) for b in boxes} == {(0, 0), (0, 1), (1, 0), (1, 1)}
  starts = {b[0] for b in boxes}
  assert {c for c in starts if c in cols} and {c for c in starts if c - 1 in cols} and {c for c in starts if c + 1 in cols}      # on, after, before a break
  assert {b[0] & 31 for b in boxes} >= ({0, 1, 31} if sx > 33 else {0, 1})      # every residue of the funnel shift the grid claims
  assert any(b[1] == sx and (b[0] & 31) for b in boxes)      # the last input word has no right neighbour, and the shift is not 0
  if sx >= 64:
    assert 31 in cols and 32 in cols and any(b[0] <= 31 and b[1] > 32 for b in boxes)      # a break at bit 31, the next at bit 0
  diagonal = volumes.edge_diagonal(sx)
  assert 0 < len(diagonal) < len(boxes) and set(diagonal) <= set(boxes)


def test_carried_labels_are_what_they_say():
  vol = volumes.carried()
  assert vol.shape == volumes.CARRIED_SHAPE
  for y in range(3):
    for z in range(2):
      assert _changes(vol[:, y, z]) == volumes.CARRIED_BREAKS
  assert volumes.CARRIED_BREAKS[1] - volumes.CARRIED_BREAKS[0] > 64 and volumes.CARRIED_BREAKS[0] < 32
  for b in volumes.CARRIED_BOXES:
    assert crop_numpy.in_bounds(b, vol.shape) and volumes.CARRIED_BREAKS[0] < 32 <= b[0] < volumes.CARRIED_BREAKS[1]      # begins inside the long run, past its first word
  assert {b[0] >> 5 for b in volumes.CARRIED_BOXES} == {1, 2}      # second and third word
  assert any(b[1] <= volumes.CARRIED_BREAKS[1] for b in volumes.CARRIED_BOXES) and any(b[1] > volumes.CARRIED_BREAKS[1] for b in volumes.CARRIED_BOXES)


@pytest.mark.parametrize("name,dtype,row,wants", volumes.HAND, ids=[c[0] for c in volumes.HAND])
def test_restatement_hand_built_rows(name, dtype, row, wants):
  assert len(wants) == len(volumes.HAND_OFFSETS) and row[0] == row[1]      # offset 1 is inside the first run
  for x0 in volumes.HAND_PLACES:
    vol = volumes.hand(dtype, row, x0)
    assert vol.shape == (x0 + len(row), 3, 2) and vol.dtype == dtype and vol[x0:, 1, 0].tolist() == list(row)
    for offset, want in zip(volumes.HAND_OFFSETS, wants):
      box = volumes.hand_box(row, x0, offset)
      assert crop_numpy.in_bounds(box, vol.shape) and len(want) == len(row) - offset
      out = crop_numpy.crop(vol, box)
      assert out[:, 0, 0].tolist() == list(want), (name, x0, offset)
      assert (out[:, 1, :] == volumes.HAND_BACKGROUND).all() and (out[:, :, 1] == volumes.HAND_BACKGROUND).all()
  assert any(x0 + o < 32 < x0 + len(row) for x0 in volumes.HAND_PLACES for o in volumes.HAND_OFFSETS if (x0 + o) & 31)      # across the first word's end


def test_first_rows_are_what_they_say():
  vol = volumes.first_rows()
  assert vol.shape == volumes.FIRST_SHAPE
  y, z = volumes.FIRST_Y, volumes.FIRST_Z
  assert (vol[:, y, :] != vol[:, y - 1, :]).all() and (vol[:, :, z] != vol[:, :, z - 1]).all()      # a boundary exactly there
  assert (vol[:, y + 1, z] != vol[:, y, z]).any() and (vol[:, y + 1, z] == vol[:, y, z]).any()
  for b in volumes.FIRST_BOXES:
    assert crop_numpy.in_bounds(b, vol.shape)
  assert sum(b[2] == y for b in volumes.FIRST_BOXES) >= 3 and sum(b[4] == z for b in volumes.FIRST_BOXES) >= 3
  # the wrap-around pairs are the box's own: the pixel before a box row's first is not the pixel before it in the input
  b = volumes.FIRST_BOXES[0]
  out = crop_numpy.crop(vol, b)
  assert out[-1, 0, 0] != vol[b[0] - 1, b[2] + 1, b[4]] or out[-1, 0, 0] != out[0, 1, 0]


@pytest.mark.parametrize("n", volumes.COUNTS)
def test_label_counts_are_what_they_say(n, checker):
  vol = volumes.counted()
  assert vol.dtype == np.uint16 and np.unique(vol).size == 320 and int(vol.max()) == 319
  box = volumes.count_box(n)
  assert crop_numpy.in_bounds(box, vol.shape)
  out = crop_numpy.crop(vol, box)
  left = np.unique(out)
  assert left.size == n and int(left.max()) == n - 1 and 319 not in left.tolist()
  binary = checker.compress(out)
  head = crackle_amd.header(binary)
  assert crackle_amd.num_labels(binary) == n and head.data_width == 2
  assert head.stored_data_width == (1 if n <= 256 else 2)
  assert crackle_amd.header(checker.compress(vol)).stored_data_width == 2      # the input's own: the box lost the largest label
  # the key width, in the bytes of the flat label section: 8 bytes of count, n stored labels, then per slice a component
  # count, and one key per component
  # (two bytes each: a slice has 2 n pixels) and one key per component
  components = 2 * n      # n columns of two equal rows in each of two slices
  keys = head.num_label_bytes - 8 - n * head.stored_data_width - 2 * 2
  assert keys % components == 0 and keys // components == (1 if n <= 255 else 2)      # (the width of the COUNT n, not of n - 1)


def test_format_flips_are_what_they_say(checker):
  busy, smooth = volumes.format_flip(True), volumes.format_flip(False)
  assert permissible(busy) and not permissible(smooth)
  for box in volumes.FORMAT_BOXES:
    assert crop_numpy.in_bounds(box, busy.shape)
    in_busy, in_smooth = crop_numpy.crop(busy, box), crop_numpy.crop(smooth, box)
    assert not permissible(in_busy) and permissible(in_smooth)
    assert np.unique(in_busy).size == 2 and np.unique(in_smooth).size == 5
    formats = [crackle_amd.header(checker.compress(v)).crack_format for v in (busy, in_busy, smooth, in_smooth)]
    assert formats == [1, 0, 0, 1]      # PERMISSIBLE is 1


def test_widths_and_generated_are_what_they_say():
  for dtype in (np.uint8, np.uint16, np.uint32, np.uint64):
    vol = volumes.for_dtype(dtype)
    assert vol.dtype == dtype and vol.shape == volumes.WIDTH_SHAPE and crop_numpy.in_bounds(volumes.WIDTH_BOX, vol.shape)
    out = crop_numpy.crop(vol, volumes.WIDTH_BOX)
    assert 5 < np.unique(out).size and crop_numpy.x_runs(out) > out.shape[1] * out.shape[2]
    if dtype == np.uint64:
      labels = np.unique(out).tolist()
      assert labels[-1] == volumes.TOP == 2**64 - 1 and any((1 << 32) < v < volumes.TOP for v in labels)
  for i, (shape, order, box) in enumerate(volumes.GENERATED):
    vol, b = volumes.generated(i)
    assert b == box and vol.shape == shape and vol.flags.c_contiguous == (order == "C") and vol.flags.f_contiguous == (order == "F")
    assert crop_numpy.in_bounds(box, shape) and box[0] & 31 and box[2] and box[4]      # off-centre, not word-aligned
    out = crop_numpy.crop(vol, box)
    assert 10 < np.unique(out).size < np.unique(vol).size + 1 and (out == 0).any()
    assert out.flags.c_contiguous == (order == "C")


def test_other_boxes_are_what_they_say():
  vol, box = volumes.many_words()
  out = crop_numpy.crop(vol, box)
  assert out.shape[0] >= 160 and out.shape[1] >= 60 and out.shape[2] >= 3 and -(-out.shape[0] // 32) * out.shape[1] > 256
  assert all(o < s for o, s in zip(out.shape, vol.shape)) and box[0] & 31
  vol, box = volumes.strip_path()
  assert crop_numpy.crop(vol, box).shape == (320, 288, 5) and all(o < s for o, s in zip((320, 288, 5), vol.shape))
  vol, box = volumes.run_pipeline()
  assert vol.shape == (32900, 3, 2) and crop_numpy.crop(vol, box).shape == (32800, 3, 2) and vol.dtype == np.uint8
  shape = volumes.GENERATED[0][0]
  mixed = volumes.MIXED_BOXES
  assert all(crop_numpy.in_bounds(b, shape) for b in mixed)
  assert len(set(mixed)) == len(mixed) - 1      # one duplicate
  assert sum(1 for b in mixed if 0 in (b[1] - b[0], b[3] - b[2], b[5] - b[4])) == 1      # one empty box
  live = [b for b in mixed if b[1] > b[0]]
  assert [b[4] for b in live] != sorted(b[4] for b in live) and len({(b[1] - b[0], b[3] - b[2], b[5] - b[4]) for b in live}) >= 4
  assert min(b[4] for b in live) == 0 and max(b[5] for b in live) == shape[2]


# ---- the surface -------------------------------------------------------------------------------------------------------
def test_surface():
  assert crackle_amd.crop is array.crop is crop and crackle_amd.crop_boxes is array.crop_boxes is crop_boxes
  assert crackle_amd.chunks is array.chunks is chunks and crackle_amd.chunk_boxes is array.chunk_boxes
  for name in ("crop", "crop_boxes", "chunks", "chunk_boxes"):
    assert name in crackle_amd.__all__
  for fn, first in ((crop, "slices"), (crop_boxes, "boxes"), (chunks, "chunk_size")):
    sig = inspect.signature(fn)
    assert list(sig.parameters) == ["binary", first, "markov_model_order", "device"] and [p.default for p in sig.parameters.values()][2:] == [None, 0]
  assert list(inspect.signature(chunk_boxes).parameters) == ["shape", "chunk_size"]
  assert list(inspect.signature(crackle_amd.CrackleArray.crop).parameters) == ["self", "slices"]
  assert list(inspect.signature(crackle_amd.CrackleArray.crop_boxes).parameters) == ["self", "boxes"]
  assert list(inspect.signature(crackle_amd.CrackleArray.chunks).parameters) == ["self", "chunk_size"]
  text = open(os.path.join(ROOT, "include", "crackle_amd.h")).read()
  assert re.search(r"\bint\s+ckl_crop\s*\(\s*const uint8_t\*\s*buf,\s*uint64_t n,\s*int64_t x0,\s*int64_t x1,\s*int64_t y0,\s*int64_t y1,\s*int64_t z0,\s*int64_t z1,\s*"
                   r"int flags[^,]*,\s*int markov_model_order[^,]*,\s*int device,\s*uint8_t\*\*\s*out,\s*uint64_t\*\s*out_len\s*\)", text)
  assert re.search(r"\bint\s+ckl_crop_boxes\s*\(\s*const uint8_t\*\s*buf,\s*uint64_t n,\s*const int64_t\*\s*boxes[^,]*,\s*uint64_t n_boxes,\s*"
                   r"int flags[^,]*,\s*int markov_model_order[^,]*,\s*int device,\s*uint8_t\*\*\s*outs,\s*uint64_t\*\s*out_lens\s*\)", text)
  lib = C.CDLL(_lib.LIB_PATH)
  assert hasattr(lib, "ckl_crop") and hasattr(lib, "ckl_crop_boxes") and "ckl_crop" in _lib.EXPORTS and "ckl_crop_boxes" in _lib.EXPORTS
  assert _lib.lib().ckl_abi_version() == 1      # entries were added, none changed
  for fn in (crop, crop_boxes):
    doc = " ".join(fn.__doc__.split())
    assert "decompress_range raises" in doc and "never looked at" in doc, fn.__name__      # what a session's z-range means for damage
  doc = " ".join(crop.__doc__.split())
  for words in ("byte for byte", "FLAT labels, format version 1", "keeps its axis at size 1", "recompress(binary)", "29-byte"):
    assert words in doc, words


def test_array_methods_pass_on(monkeypatch):
  calls = []
  binary = golden()["c0_voronoi_u8"]
  monkeypatch.setattr(array, "crop", lambda b, s, **kw: calls.append(("crop", b, s, kw)) or b)
  monkeypatch.setattr(array, "crop_boxes", lambda b, boxes, **kw: calls.append(("crop_boxes", b, boxes, kw)) or [b, b])
  monkeypatch.setattr(array, "chunks", lambda b, size, **kw: calls.append(("chunks", b, size, kw)) or {(0, 0, 0): b})
  arr = crackle_amd.CrackleArray(binary, device=0)
  out = arr.crop(np.s_[1:3, :, 2])
  assert type(out) is crackle_amd.CrackleArray and out is not arr and out.binary == binary
  outs = arr.crop_boxes([np.s_[:2], np.s_[2:]])
  assert [type(o) for o in outs] == [crackle_amd.CrackleArray] * 2
  grid = arr.chunks((8, 8, 8))
  assert list(grid) == [(0, 0, 0)] and type(grid[(0, 0, 0)]) is crackle_amd.CrackleArray
  assert calls == [("crop", binary, np.s_[1:3, :, 2], dict(device=0)), ("crop_boxes", binary, [np.s_[:2], np.s_[2:]], dict(device=0)), ("chunks", binary, (8, 8, 8), dict(device=0))]


# ---- what the host answers without a device ----------------------------------------------------------------------------
def _entries(binary):
  L = _lib.lib()
  out, n = C.c_void_p(), C.c_uint64()

  def one(box, flags=0, order=-1):
    rc = L.ckl_crop(binary, len(binary), *box, flags, order, 0, C.byref(out), C.byref(n))
    return rc, L.ckl_last_error().decode(), out, n

  def many(boxes, flags=0, order=-1):
    k = len(boxes)
    flat = (C.c_int64 * max(1, 6 * k))(*[v for b in boxes for v in b])
    outs, lens = (C.c_void_p * max(1, k))(), (C.c_uint64 * max(1, k))()
    rc = L.ckl_crop_boxes(binary, len(binary), flat, k, flags, order, 0, outs, lens)
    return rc, L.ckl_last_error().decode(), outs, lens

  return one, many


def test_index_errors_are_cutouts(checker):
  binary = golden()["c0_voronoi_u8"]
  head = crackle_amd.header(binary)
  sx = head.sx
  for expr in (np.s_[0:sx + 1], np.s_[-sx - 1:], np.s_[::-1], np.s_[::0], np.s_[..., 1, ...], sx, -sx - 1, np.s_[0, 0, 0, 0], np.s_[1.5], np.s_[[1, 2]]):
    with pytest.raises(Exception) as theirs:
      array.normalize_index(expr, (head.sx, head.sy, head.sz))
    for call in (lambda: crop(binary, expr), lambda: crop_boxes(binary, [np.s_[:], expr]), lambda: crackle_amd.CrackleArray(binary).crop(expr)):
      with pytest.raises(type(theirs.value), match=re.escape(str(theirs.value))):
        call()
  # steps
  for expr in (np.s_[::2], np.s_[:, 1:9:3], np.s_[..., ::4], np.s_[0:1:2]):
    for call in (lambda: crop(binary, expr), lambda: crop_boxes(binary, [expr]), lambda: crackle_amd.CrackleArray(binary).crop(expr)):
      with pytest.raises(ValueError, match="crop: steps other than 1 are not supported"):
        call()
  # the order
  with pytest.raises(ValueError, match="crop: markov_model_order must not be negative"):
    crop(binary, np.s_[:], markov_model_order=-1)
  with pytest.raises(ValueError) as seen:
    crackle_amd.recompress(binary, markov_model_order=16)
  with pytest.raises(ValueError, match=re.escape(str(seen.value))):      # the road's own error, before a device is asked for
    crop(binary, np.s_[:], markov_model_order=16)
  # signed streams
  signed = as_signed(binary)
  assert crackle_amd.header(signed).signed
  for call in (lambda: crop(signed, np.s_[:]), lambda: crop_boxes(signed, [np.s_[:2]]), lambda: chunks(signed, (8, 8, 8)), lambda: crackle_amd.CrackleArray(signed).crop(np.s_[:])):
    with pytest.raises(TypeError, match="Signed integer data types are not currently supported."):
      call()
  one, many = _entries(signed)
  rc, said, out, n = one((0, 1, 0, 1, 0, 1))
  assert rc == _lib.CKL_ERR_ARG and "Signed integer data types are not currently supported." in said and out.value is None
  assert crop_boxes(binary, []) == [] and crackle_amd.CrackleArray(binary).crop_boxes([]) == []


@pytest.mark.parametrize("order", ["F", "C"])
def test_empty_boxes_are_header_only(checker, order):
  x, y, z = np.meshgrid(np.arange(5), np.arange(4), np.arange(3), indexing="ij")
  vol = np.array((x >= 2) + 2 * (y >= 2) + 4 * (z >= 1), np.uint16, order=order)
  binary = checker.compress(vol, fortran_order=(order == "F"), markov_model_order=3)
  assert crackle_amd.header(binary).markov_model_order == 3
  for expr, shape in ((np.s_[2:2], (0, 4, 3)), (np.s_[:, 4:4, 1:2], (5, 0, 1)), (np.s_[1:3, :, 0:0], (2, 4, 0)), (np.s_[5:5, 0:0, 3:3], (0, 0, 0)), (np.s_[1, 2:2], (1, 0, 3))):
    got = crop(binary, expr)
    assert len(got) == 29
    assert got == checker.compress(np.zeros(shape, np.uint16, order=order), fortran_order=(order == "F"), markov_model_order=3), shape
    head = crackle_amd.header(got)
    assert (head.sx, head.sy, head.sz) == shape and head.data_width == 2 and head.fortran_order == (order == "F")
    assert crop(binary, expr, markov_model_order=0) == checker.compress(np.zeros(shape, np.uint16, order=order), fortran_order=(order == "F"))
    assert crackle_amd.CrackleArray(binary).crop(expr).binary == got
  both = crop_boxes(binary, [np.s_[2:2], np.s_[:, :, 3:3]])
  assert both == [crop(binary, np.s_[2:2]), crop(binary, np.s_[:, :, 3:3])]
  one, many = _entries(binary)
  rc, _, out, n = one((1, 1, 0, 4, 0, 3))
  try:
    assert rc == _lib.CKL_OK and C.string_at(out.value, n.value) == crop(binary, np.s_[1:1])
  finally:
    _lib.lib().ckl_free(out)
  # a stream without voxels: every box of it is empty
  nothing = checker.compress(np.zeros((4, 0, 3), np.uint8, order="F"))
  assert crop(nothing, np.s_[1:3]) == checker.compress(np.zeros((2, 0, 3), np.uint8, order="F"))
  assert chunks(nothing, (2, 2, 2)) == {}


def test_the_c_entries_refuse_on_the_host():
  binary = golden()["c0_voronoi_u8"]
  head = crackle_amd.header(binary)
  sx, sy, sz = head.sx, head.sy, head.sz
  one, many = _entries(binary)
  # no boxes: nothing is touched, whatever else is passed
  L = _lib.lib()
  assert L.ckl_crop_boxes(binary, len(binary), None, 0, 0, -1, 0, None, None) == _lib.CKL_OK
  assert L.ckl_crop_boxes(None, 0, None, 0, 0, -1, 0, None, None) == _lib.CKL_OK
  rc, _, outs, lens = many([])
  assert rc == _lib.CKL_OK and outs[0] is None and lens[0] == 0
  # flags
  for flags in (1, 2, -1):
    rc, said, out, n = one((0, 1, 0, 1, 0, 1), flags=flags)
    assert rc == _lib.CKL_ERR_ARG and "crop: flags must be 0" in said
    rc, said, outs, lens = many([(0, 1, 0, 1, 0, 1)], flags=flags)
    assert rc == _lib.CKL_ERR_ARG and "crop: flags must be 0" in said and outs[0] is None
    assert L.ckl_crop_boxes(binary, len(binary), None, 0, flags, -1, 0, None, None) == _lib.CKL_ERR_ARG
  # boxes outside the volume, with the axis named; nothing is clamped
  for axis, box in (("x", (0, sx + 1, 0, sy, 0, sz)), ("x", (-1, 2, 0, sy, 0, sz)), ("x", (3, 2, 0, sy, 0, sz)),
                    ("y", (0, sx, 0, sy + 1, 0, sz)), ("y", (0, sx, 5, 4, 0, sz)), ("z", (0, sx, 0, sy, 0, sz + 1)), ("z", (0, sx, 0, sy, -2, 1))):
    rc, said, out, n = one(box)
    assert rc == _lib.CKL_ERR_ARG and ("crop: %s range %d - %d is not an ascending range inside 0 - " % (axis, box["xyz".index(axis) * 2], box["xyz".index(axis) * 2 + 1])) in said, said
    assert out.value is None and n.value == 0
    # every box is checked before any work: an empty box ahead of the bad one has been handed out by nobody
    rc, said, outs, lens = many([(0, 0, 0, 1, 0, 1), box])
    assert rc == _lib.CKL_ERR_ARG and ("crop: %s range" % axis) in said and outs[0] is None and outs[1] is None and lens[0] == lens[1] == 0
  # the order, null pointers, a stream too short
  rc, said, out, n = one((0, 1, 0, 1, 0, 1), order=16)
  assert rc == _lib.CKL_ERR_ARG and "markov_model_order must be in [0, 15]" in said
  k = len(binary)
  out, n = C.c_void_p(), C.c_uint64()
  assert L.ckl_crop(None, 0, 0, 1, 0, 1, 0, 1, 0, -1, 0, C.byref(out), C.byref(n)) == _lib.CKL_ERR_ARG
  assert L.ckl_crop(binary, k, 0, 1, 0, 1, 0, 1, 0, -1, 0, None, C.byref(n)) == _lib.CKL_ERR_ARG
  assert L.ckl_crop(binary, k, 0, 1, 0, 1, 0, 1, 0, -1, 0, C.byref(out), None) == _lib.CKL_ERR_ARG
  assert L.ckl_crop(binary[:10], 10, 0, 1, 0, 1, 0, 1, 0, -1, 0, C.byref(out), C.byref(n)) != _lib.CKL_OK
  assert out.value is None and n.value == 0
