"""GPU tests of crackle_amd.crop, crop_boxes and chunks (ckl_crop_boxes: one decode session's run tables over the boxes'
z-range -> k_erode_run_labels once, then per box k_crop_cuts, k_crop_labels, k_pool_planes -> the encoder's crack and
label stages; crackle_amd/csrc/ckl_crop.hpp and ckl_recompress.hip).

The check throughout: the result equals the checker's compress of the restated box (tests/crop_numpy.py, worked from the
INPUT array) byte for byte under the requested markov order (default: the input's) and the input's order flag; it
decodes, here and with the checker, to that array in the right dtype and memory order; crackle_amd.ok() accepts it; its
labels are the array's; its header is FLAT, version 1, with the input's data width.  The volumes and boxes and what each
of them is about: tests/crop_volumes.py, pinned on the CPU by tests/test_crop_cpu.py."""
import os
import re

import numpy as np
import pytest

import crackle_amd
import crop_numpy
import crop_volumes as volumes
import dust_numpy
import erode_volumes
import stream_kinds
from recompress_volumes import permissible
from crackle_amd import crop, crop_boxes, chunks      # (the feature under test: without it nothing here runs)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ENCODINGS = [dict(), dict(allow_pins=True), dict(markov_model_order=5)]
ENCODING_IDS = ["flat", "pins", "markov5"]
S = crop_numpy.slices


def _compress(vol, checker, **kw):
  return checker.compress(vol, fortran_order=bool(vol.flags.f_contiguous), **kw)


def _verify(got, stream, expected, checker, order=None):
  """got: what crop gave for the box of `stream` whose restatement is `expected` (in the memory order of the stream's flag)."""
  head = crackle_amd.header(stream)
  m = head.markov_model_order if order is None else order
  want = checker.compress(expected, fortran_order=head.fortran_order, markov_model_order=m)
  assert isinstance(got, bytes)
  assert got == want, f"{expected.shape} {expected.dtype} order={order}"
  out = crackle_amd.header(got)
  # (the order is in the bytes compared above: compress itself writes order 0 into the stream of a volume without cracks)
  assert out.label_format == 0 and out.format_version == 1 and out.fortran_order == head.fortran_order
  assert out.data_width == expected.dtype.itemsize == head.data_width and not out.signed
  assert (out.sx, out.sy, out.sz) == expected.shape
  mine = crackle_amd.decompress(got)
  assert mine.dtype == expected.dtype and np.array_equal(mine, expected)
  if expected.flags.f_contiguous != expected.flags.c_contiguous:
    assert mine.flags.f_contiguous == expected.flags.f_contiguous
  theirs = checker.decompress(got).reshape(expected.shape, order="F" if head.fortran_order else "C")
  assert theirs.dtype == expected.dtype and np.array_equal(theirs, expected)
  assert crackle_amd.ok(got)
  assert np.array_equal(np.sort(np.asarray(crackle_amd.labels(got))), np.unique(expected))
  return got


def _check(stream, vol, box, checker, order=None):
  """vol: what `stream` decodes to, in the memory order of its flag."""
  return _verify(crop(stream, S(box), markov_model_order=order), stream, crop_numpy.crop(vol, box), checker, order=order)


def _crop_and_check(vol, box, checker, order=None, **kw):
  return _check(_compress(vol, checker, **kw), vol, box, checker, order=order)


# ---- word edges --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sx", volumes.EDGE_SX)
def test_word_edges(sx, checker):
  """The full grid through ONE crop_boxes call, byte for byte; a diagonal subset one by one, with all of the checks."""
  vol = volumes.edges(sx)
  stream = _compress(vol, checker)
  boxes = volumes.edge_boxes(sx)
  got = crop_boxes(stream, [S(b) for b in boxes])
  assert len(got) == len(boxes)
  for b, g in zip(boxes, got):
    assert g == checker.compress(crop_numpy.crop(vol, b), fortran_order=True), (sx, b)
  at = {b: g for b, g in zip(boxes, got)}
  for b in volumes.edge_diagonal(sx):
    assert _check(stream, vol, b, checker) == at[b], (sx, b)


def test_carried_labels(checker):
  vol = volumes.carried()
  stream = _compress(vol, checker)
  for b in volumes.CARRIED_BOXES:
    got = _check(stream, vol, b, checker)
    assert int(crackle_amd.decompress(got)[0, 0, 0]) == int(vol[2 * 16, b[2], b[4]])      # the label of the run that began two words back
  assert crop_boxes(stream, [S(b) for b in volumes.CARRIED_BOXES]) == [crop(stream, S(b)) for b in volumes.CARRIED_BOXES]


@pytest.mark.parametrize("name,dtype,row,wants", volumes.HAND, ids=[c[0] for c in volumes.HAND])
def test_hand_built_rows(name, dtype, row, wants, checker):
  for x0 in volumes.HAND_PLACES:
    vol = volumes.hand(dtype, row, x0)
    stream = _compress(vol, checker)
    for offset, want in zip(volumes.HAND_OFFSETS, wants):
      got = _check(stream, vol, volumes.hand_box(row, x0, offset), checker)
      assert crackle_amd.decompress(got)[:, 0, 0].tolist() == list(want)      # (the literal answer)


def test_first_row_and_first_slice(checker):
  vol = volumes.first_rows()
  stream = _compress(vol, checker, markov_model_order=2)
  for b in volumes.FIRST_BOXES:
    _check(stream, vol, b, checker)
  assert crop_boxes(stream, [S(b) for b in volumes.FIRST_BOXES]) == [crop(stream, S(b)) for b in volumes.FIRST_BOXES]


# ---- label counts, crack formats, data widths --------------------------------------------------------------------------
@pytest.mark.parametrize("n", volumes.COUNTS)
def test_label_counts_around_a_byte_of_index(n, checker):
  vol = volumes.counted()
  stream = _compress(vol, checker)
  assert crackle_amd.num_labels(stream) == 320 and crackle_amd.header(stream).stored_data_width == 2
  got = _check(stream, vol, volumes.count_box(n), checker)
  assert crackle_amd.num_labels(got) == n
  assert 319 not in crackle_amd.labels(got).tolist()      # the input's largest label is not in the box
  head = crackle_amd.header(got)
  assert head.stored_data_width == (1 if n <= 256 else 2) and head.data_width == 2
  keys = head.num_label_bytes - 8 - n * head.stored_data_width - 2 * 2      # (tests/test_crop_cpu.py: the same sum on the checker's bytes)
  assert keys == 2 * n * (1 if n <= 255 else 2)


def _format_bit(stream):
  return crackle_amd.header(stream).crack_format == 1


def test_the_crack_format_follows_the_box(checker):
  seen = []
  for busy_first in (True, False):
    vol = volumes.format_flip(busy_first)
    stream = _compress(vol, checker)
    assert _format_bit(stream) == permissible(vol) == busy_first
    for b in volumes.FORMAT_BOXES:
      got = _check(stream, vol, b, checker)
      assert _format_bit(got) == permissible(crop_numpy.crop(vol, b)) == (not busy_first)      # another format than the input's
      seen.append((_format_bit(stream), _format_bit(got)))
  assert set(seen) == {(True, False), (False, True)}


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.uint64], ids=lambda d: np.dtype(d).name)
def test_every_unsigned_width(dtype, checker):
  vol = volumes.for_dtype(dtype)
  got = _crop_and_check(vol, volumes.WIDTH_BOX, checker, markov_model_order=2)
  assert crackle_amd.header(got).data_width == np.dtype(dtype).itemsize
  if dtype == np.uint64:
    assert int(crackle_amd.decompress(got).max()) == volumes.TOP


# ---- generated ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=range(len(volumes.GENERATED)), ids=["x".join(map(str, g[0])) + g[1] for g in volumes.GENERATED])
def generated(request):
  vol, box = volumes.generated(request.param)
  vol.setflags(write=False)
  return vol, box


@pytest.mark.parametrize("kw", ENCODINGS, ids=ENCODING_IDS)
def test_generated(generated, kw, checker):
  vol, box = generated
  stream = _compress(vol, checker, **kw)
  assert crackle_amd.header(stream).label_format == (2 if kw.get("allow_pins") else 0) and crackle_amd.header(stream).fortran_order == bool(vol.flags.f_contiguous)
  got = _check(stream, vol, box, checker)
  assert crackle_amd.header(got).markov_model_order == kw.get("markov_model_order", 0)      # the input's


@pytest.mark.parametrize("order", [0, 3])
def test_explicit_markov_order(generated, order, checker):
  vol, box = generated
  got = _crop_and_check(vol, box, checker, order=order, markov_model_order=5)
  assert crackle_amd.header(got).markov_model_order == order
  stream = _compress(vol, checker, markov_model_order=5)
  assert crop_boxes(stream, [S(box)], markov_model_order=order) == [got]
  assert list(chunks(stream, vol.shape, markov_model_order=order).values()) == [crackle_amd.recompress(stream, markov_model_order=order)]


@pytest.mark.parametrize("shape,box", [((37, 1, 1), (5, 36, 0, 1, 0, 1)), ((1, 6, 5), (0, 1, 1, 5, 2, 4)), ((1, 1, 1), (0, 1, 0, 1, 0, 1)), ((65, 2, 2), (64, 65, 1, 2, 0, 2)),
                                       ((70, 50, 13), (69, 70, 49, 50, 12, 13)), ((70, 50, 13), (31, 33, 0, 50, 0, 13))], ids=lambda s: "x".join(map(str, s)))
def test_small_shapes(shape, box, checker):
  vol = volumes.generated(0)[0][:shape[0], :shape[1], :shape[2]].copy(order="F")
  _crop_and_check(vol, box, checker)


def test_int_indices_keep_their_axes(generated, checker):
  vol, _ = generated
  stream = _compress(vol, checker)
  for expr, box in ((np.s_[5], (5, 6, 0, vol.shape[1], 0, vol.shape[2])), (np.s_[..., -1], (0, vol.shape[0], 0, vol.shape[1], vol.shape[2] - 1, vol.shape[2])),
                    (np.s_[3:40, 7, 2], (3, 40, 7, 8, 2, 3)), (np.s_[-30:-2, :, 4:9], (vol.shape[0] - 30, vol.shape[0] - 2, 0, vol.shape[1], 4, 9))):
    got = _verify(crop(stream, expr), stream, crop_numpy.crop(vol, box), checker)
    assert crackle_amd.decompress(got).ndim == 3


# ---- both label paths of the encoder, and the profile line -------------------------------------------------------------
FIELDS = ["tables", "crop_planes", "graph", "cracks", "labels", "assembly", "k_crop_device", "pieces"]


def _profiled(capfd, monkeypatch, stream, boxes):
  """crop_boxes under CKL_PROFILE: the streams, per box the marks of the encoder's label stage and the pieces."""
  monkeypatch.setenv("CKL_PROFILE", "1")
  capfd.readouterr()
  got = crop_boxes(stream, [S(b) for b in boxes])
  monkeypatch.delenv("CKL_PROFILE", raising=False)
  err = capfd.readouterr().err.splitlines()
  mine = [l for l in err if l.startswith("[ckl crop host ms]")]
  assert len(mine) == len(boxes), err      # one line per box
  enc = [l for l in err if l.startswith("[ckl encode host ms]")]
  assert len(enc) == len(boxes), err
  marks, pieces = [], []
  for k, line in enumerate(mine):
    fields = dict(w.split("=") for w in line.split()[4:])
    assert list(fields) == FIELDS, line
    assert float(fields["crop_planes"]) > 0 and float(fields["k_crop_device"]) > 0
    assert (float(fields["tables"]) > 0) == (k == 0), line      # the shared run stands on the first box's line
    pieces.append(int(fields["pieces"]))
    marks.append(sorted(w.split("=")[0] for w in enc[k].split() if w.startswith("f:")))
  return got, marks, pieces


def test_many_workgroups_of_words(checker, monkeypatch, capfd):
  vol, box = volumes.many_words()
  stream = _compress(vol, checker)
  got = _check(stream, vol, box, checker)
  other = (1, 164, 0, 62, 2, 5)      # the same shape elsewhere: the second turn of one encode session
  again, _, pieces = _profiled(capfd, monkeypatch, stream, [box, other, box])
  assert again[0] == again[2] == got and again[1] == _check(stream, vol, other, checker)
  assert pieces == [crop_numpy.x_runs(crop_numpy.crop(vol, b)) for b in (box, other, box)]
  assert pieces[0] > (box[3] - box[2]) * (box[5] - box[4])


def test_strip_path(checker, monkeypatch, capfd):
  vol, box = volumes.strip_path()
  stream = _compress(vol, checker)
  monkeypatch.delenv("CKL_ENC_LABEL_RUNS", raising=False)
  expected = crop_numpy.crop(vol, box)
  got = _check(stream, vol, box, checker)
  again, marks, pieces = _profiled(capfd, monkeypatch, stream, [box])
  assert again == [got] and "f:enqueue_strips" in marks[0] and "f:wait_strips" in marks[0], marks
  assert pieces == [crop_numpy.x_runs(expected)]
  # the same box with the run pipeline forced
  monkeypatch.setenv("CKL_ENC_LABEL_RUNS", "1")
  again, marks, pieces = _profiled(capfd, monkeypatch, stream, [box])
  monkeypatch.delenv("CKL_ENC_LABEL_RUNS")
  assert again == [got] and "f:enqueue_runs" in marks[0] and "f:wait_runs" in marks[0], marks
  assert pieces == [crop_numpy.x_runs(expected)]


def test_run_pipeline(checker, monkeypatch, capfd):
  vol, box = volumes.run_pipeline()
  stream = _compress(vol, checker)
  monkeypatch.delenv("CKL_ENC_LABEL_RUNS", raising=False)
  got = _check(stream, vol, box, checker)
  again, marks, pieces = _profiled(capfd, monkeypatch, stream, [box])
  assert again == [got] and "f:enqueue_runs" in marks[0] and "f:wait_runs" in marks[0], marks
  assert pieces == [crop_numpy.x_runs(crop_numpy.crop(vol, box))]


# ---- every kind of stream ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kinds(checker):
  vol = stream_kinds.volume_a()
  return {k.name: k for k in stream_kinds.kinds_host(vol, checker) + stream_kinds.kinds_device(vol, checker)}


def _off_centre(shape):
  """An odd-offset box that is no whole plane and not word-aligned; of a thin volume, all of its depth but the first slice."""
  sx, sy, sz = shape
  return (min(7, sx - 1), sx - 3 if sx > 12 else sx, min(3, sy - 1), sy - 2 if sy > 8 else sy, 1 if sz > 1 else 0, sz - 1 if sz > 3 else sz)


@pytest.mark.parametrize("name", stream_kinds.HOST_KINDS + stream_kinds.DEVICE_KINDS)
def test_every_stream_kind(name, kinds, checker):
  kind = kinds[name]
  _check(kind.stream, kind.expected, _off_centre(kind.expected.shape), checker)


def test_version_0_stream(checker):
  with np.load(os.path.join(HERE, "golden", "v0.npz")) as z:
    b0 = z[sorted(k for k in z.files if "." not in k)[0]].tobytes()
  head = crackle_amd.header(b0)
  assert head.format_version == 0 and not head.signed
  arr = checker.decompress(b0).reshape((head.sx, head.sy, head.sz), order="F" if head.fortran_order else "C")
  _check(b0, arr, _off_centre(arr.shape), checker)
  assert crop(b0, np.s_[:]) == crackle_amd.recompress(b0)


# ---- false boundaries --------------------------------------------------------------------------------------------------
def _with_and_without_false_boundaries(dirty, volume, checker):
  """dirty: a stream of `volume` with false boundaries.  Its boxes are those of its recompressed form."""
  clean = crackle_amd.recompress(dirty)
  assert len(clean) < len(dirty)
  for box in (volumes.GENERATED[0][2], (0, 33, 0, 50, 0, 13)):
    assert _check(dirty, volume, box, checker) == crop(clean, S(box))


def test_false_boundaries_of_remap(checker):
  vol = erode_volumes.merging()
  dirty = crackle_amd.remap(_compress(vol, checker), erode_volumes.MERGE, preserve_missing_labels=True)
  _with_and_without_false_boundaries(dirty, erode_volumes.merged(vol), checker)


def test_false_boundaries_of_dust(checker):
  vol = erode_volumes.merging()
  dusted, removed = dust_numpy.dust(vol, 300, 26)
  assert removed > 0
  dirty = crackle_amd.dust(_compress(vol, checker), 300, connectivity=26)
  _with_and_without_false_boundaries(dirty, np.asfortranarray(dusted), checker)


# ---- identities --------------------------------------------------------------------------------------------------------
def test_identities(generated, checker):
  vol, box = generated
  stream = _compress(vol, checker, markov_model_order=3)
  same = crackle_amd.recompress(stream)
  assert same == _compress(vol, checker, markov_model_order=3)
  assert crop(stream, np.s_[:]) == crop(stream, S((0, vol.shape[0], 0, vol.shape[1], 0, vol.shape[2]))) == same      # the whole box
  # a crop of a crop
  x0, x1, y0, y1, z0, z1 = box
  inner = (3, x1 - x0 - 5, 2, y1 - y0 - 1, 1, z1 - z0 - 2)
  both = (x0 + inner[0], x0 + inner[1], y0 + inner[2], y0 + inner[3], z0 + inner[4], z0 + inner[5])
  first = crop(stream, S(box))
  assert crop(first, S(inner)) == crop(stream, S(both)) == checker.compress(crop_numpy.crop(vol, both), fortran_order=bool(vol.flags.f_contiguous), markov_model_order=3)
  # against cutout and paste
  voxels = crackle_amd.decompress(first)
  assert np.array_equal(voxels, crackle_amd.cutout(stream, S(box)))
  assert np.array_equal(crackle_amd.decompress(crackle_amd.paste(stream, S(box), voxels)), vol)
  # against zsplit: the middle part is the crop of that z-range
  before, middle, after = crackle_amd.zsplit(stream, z0)
  assert crackle_amd.recompress(middle) == crop(stream, np.s_[:, :, z0:z0 + 1]) == crop(stream, np.s_[:, :, z0])
  # CrackleArray: the same bytes, new arrays
  arr = crackle_amd.CrackleArray(stream)
  out = arr.crop(S(box))
  assert type(out) is crackle_amd.CrackleArray and out is not arr and out.binary == first and out.shape == (x1 - x0, y1 - y0, z1 - z0)
  outs = arr.crop_boxes([S(box), S(both)])
  assert [type(o) for o in outs] == [crackle_amd.CrackleArray] * 2 and [o.binary for o in outs] == [first, crop(stream, S(both))]


def test_chunks_put_back_together(generated, checker):
  vol, _ = generated
  stream = _compress(vol, checker)
  size = (32, 32, 4)
  grid = chunks(stream, size)
  boxes = crackle_amd.chunk_boxes(vol.shape, size)
  assert boxes == crop_numpy.chunk_boxes(vol.shape, size)
  assert list(grid) == [(b[0], b[2], b[4]) for b in boxes]      # keys and order
  back = np.zeros_like(vol)
  for b in boxes:
    piece = grid[(b[0], b[2], b[4])]
    assert piece == checker.compress(crop_numpy.crop(vol, b), fortran_order=bool(vol.flags.f_contiguous)), b
    back[S(b)] = crackle_amd.decompress(piece)
  assert np.array_equal(back, vol) and np.array_equal(back, crackle_amd.decompress(stream))
  arrays = crackle_amd.CrackleArray(stream).chunks(size)
  assert list(arrays) == list(grid) and all(type(a) is crackle_amd.CrackleArray and a.binary == grid[k] for k, a in arrays.items())


# ---- an independent check through the consumers -----------------------------------------------------------------------
def test_consumers_of_a_crop(generated, checker):
  vol, box = generated
  stream = _compress(vol, checker, allow_pins=True)
  got = crop(stream, S(box))
  labels, counts = np.unique(crackle_amd.cutout(stream, S(box)), return_counts=True)
  assert crackle_amd.voxel_counts(got) == dict(zip(labels.tolist(), counts.tolist()))
  # the boxes of the labels, shifted by the box's origin, are their boxes in the input clipped to the box
  mine = crackle_amd.bounding_boxes(got, no_slice_conversion=True)
  assert sorted(mine) == labels.tolist()
  cut = crop_numpy.crop(vol, box)
  for label in labels.tolist()[:12]:
    where = np.argwhere(cut == label)
    found = [int(v) for v in mine[label]]
    assert found == where.min(axis=0).tolist() + where.max(axis=0).tolist(), label
    shifted = [v + o for v, o in zip(found, (box[0], box[2], box[4]) * 2)]
    inside = np.argwhere(vol == label)
    assert all(lo >= m for lo, m in zip(shifted[:3], inside.min(axis=0))) and all(hi <= m for hi, m in zip(shifted[3:], inside.max(axis=0)))


# ---- many boxes in one call --------------------------------------------------------------------------------------------
def test_unequal_boxes_in_one_call(checker):
  vol, _ = volumes.generated(0)
  stream = _compress(vol, checker, markov_model_order=4)
  got = crop_boxes(stream, [S(b) for b in volumes.MIXED_BOXES])
  assert len(got) == len(volumes.MIXED_BOXES)
  for b, g in zip(volumes.MIXED_BOXES, got):
    expected = crop_numpy.crop(vol, b)
    if expected.size:
      _verify(g, stream, expected, checker)
    else:
      assert len(g) == 29 and g == checker.compress(expected, markov_model_order=4)
    assert g == crop(stream, S(b))
  assert got[1] == got[4]      # the duplicate


def test_repeatable(checker):
  vol, box = volumes.many_words()
  stream = _compress(vol, checker, markov_model_order=4)
  boxes = [S(box), S((40, 70, 10, 50, 0, 5)), S(box)]
  outs = [crop_boxes(stream, boxes) for _ in range(3)]
  assert outs[0] == outs[1] == outs[2] and outs[0][0] == outs[0][2] == checker.compress(crop_numpy.crop(vol, box), markov_model_order=4)


# ---- damage ------------------------------------------------------------------------------------------------------------
def _damaged(stream, z):
  """The stream with a byte of slice z's crack codes flipped, and what decompress raises for it."""
  head = crackle_amd.header(stream)
  lens = [int.from_bytes(stream[29 + 4 * k:33 + 4 * k], "little") for k in range(head.sz)]
  codes = head.header_bytes + head.grid_index_bytes + head.num_label_bytes
  bad = bytearray(stream)
  bad[codes + sum(lens[:z]) + lens[z] // 2] ^= 0xFF
  with pytest.raises(Exception) as seen:
    crackle_amd.decompress(bytes(bad))
  assert "z=%d" % z in str(seen.value)
  return bytes(bad), seen.value


def test_a_damaged_slice_matters_inside_the_z_range_only(checker):
  """A decoder error that the library reports, as decompress reports it: no fault of the device is involved."""
  vol = erode_volumes.voronoi((48, 40, 6), dtype=np.uint16, cell=(8, 8, 2))
  stream = _compress(vol, checker)
  bad, error = _damaged(stream, 2)
  holds = (5, 40, 3, 30, 1, 4)      # z = 2 is inside, though the box is elsewhere in x and y than the flipped byte may be
  misses = (5, 40, 3, 30, 3, 6)
  below = (0, 48, 0, 40, 0, 2)
  with pytest.raises(type(error), match=re.escape(str(error))):
    crop(bad, S(holds))
  for box in (misses, below):
    assert crop(bad, S(box)) == checker.compress(crop_numpy.crop(vol, box)) == crop(stream, S(box))
  # one box of each kind: the z-range of the call holds z, nothing is returned
  with pytest.raises(type(error), match=re.escape(str(error))):
    crop_boxes(bad, [S(misses), S(holds)])
  with pytest.raises(type(error), match=re.escape(str(error))):
    crop_boxes(bad, [S(misses), S(below)])      # neither box holds z = 2, but the session's range [0, 6) does
  with pytest.raises(type(error), match=re.escape(str(error))):
    chunks(bad, (32, 32, 4))
  # the next good call is right
  assert crop_boxes(stream, [S(misses), S(holds)]) == [checker.compress(crop_numpy.crop(vol, b)) for b in (misses, holds)]
  assert crop(bad, S(misses)) == checker.compress(crop_numpy.crop(vol, misses))
