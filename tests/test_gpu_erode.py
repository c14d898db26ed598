"""GPU tests of crackle_amd.erode (ckl_erode: the decoder's run tables -> k_erode_run_labels, k_erode_terms,
k_erode_keep, k_erode_planes -> the encoder's crack and label stages; crackle_amd/csrc/ckl_erode.hpp and
ckl_recompress.hip).

The check throughout: erode(stream, ...) equals the checker's compress of the restated erosion (tests/erode_numpy.py,
worked from the INPUT array) byte for byte under the requested markov order (default: the stream's); the result
decodes, here and with the checker, to that array in the input's dtype and memory order; crackle_amd.ok() accepts it;
its labels are the array's; its header is FLAT, version 1, with the input's data width and order flag.  The volumes
and what each of them is about: tests/erode_volumes.py, pinned on the CPU by tests/test_erode_cpu.py."""
import os
import re

import numpy as np
import pytest

import crackle_amd
import dust_numpy
import erode_numpy
import erode_volumes as volumes
import fill_holes_numpy
import fill_holes_volumes
from recompress_volumes import permissible
from crackle_amd import erode      # (the feature under test: without it nothing here runs)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CONNECTIVITIES = volumes.CONNECTIVITIES
BORDERS = (True, False)
ENCODINGS = [dict(), dict(allow_pins=True), dict(markov_model_order=5)]
ENCODING_IDS = ["flat", "pins", "markov5"]


def _compress(vol, checker, **kw):
  return checker.compress(vol, fortran_order=bool(vol.flags.f_contiguous), **kw)


def _check(stream, expected, checker, conn, border, order=None):
  """expected: the restated erosion, in the memory order of the stream's flag."""
  head = crackle_amd.header(stream)
  m = head.markov_model_order if order is None else order
  want = checker.compress(expected, fortran_order=head.fortran_order, markov_model_order=m)
  got = crackle_amd.erode(stream, connectivity=conn, erode_border=border, markov_model_order=order)
  assert got == want, f"{expected.shape} {expected.dtype} connectivity={conn} erode_border={border} order={order}"
  out = crackle_amd.header(got)
  assert out.label_format == 0 and out.format_version == 1 and out.data_width == head.data_width and out.fortran_order == head.fortran_order
  mine = crackle_amd.decompress(got)
  assert mine.dtype == expected.dtype and np.array_equal(mine, expected)
  if expected.flags.f_contiguous != expected.flags.c_contiguous:
    assert mine.flags.f_contiguous == expected.flags.f_contiguous
  theirs = checker.decompress(got).reshape(expected.shape, order="F" if head.fortran_order else "C")
  assert theirs.dtype == expected.dtype and np.array_equal(theirs, expected)
  assert crackle_amd.ok(got)
  assert np.array_equal(np.sort(np.asarray(crackle_amd.labels(got))), np.unique(expected))
  return got


def _erode_and_check(vol, checker, conn, border, order=None, **kw):
  return _check(_compress(vol, checker, **kw), erode_numpy.erode(vol, conn, border), checker, conn, border, order=order)


# ---- which neighbour counts --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", volumes.NEIGHBOURS, ids=lambda o: "%+d%+d%+d" % o)
def test_which_neighbour_counts(offset, checker):
  vol = volumes.probe(offset)
  b = _compress(vol, checker)
  for conn in CONNECTIVITIES:
    got = _check(b, erode_numpy.erode(vol, conn, True), checker, conn, True)
    centre = crackle_amd.decompress(got)[volumes.PROBE_CENTRE]
    assert (centre == 1) == volumes.probe_centre_survives(offset, conn)      # (stated literally there)
    assert centre in (0, 1)


# ---- word and row edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", volumes.EDGE_VARIANTS)
@pytest.mark.parametrize("sx", volumes.EDGE_SX)
def test_word_and_row_edges(sx, variant, checker):
  """Every sy, sz of 1 .. 4 at every connectivity and both border rules, byte for byte; all of the checks on the largest."""
  for sy in volumes.EDGE_SYZ:
    for sz in volumes.EDGE_SYZ:
      vol = volumes.edges((sx, sy, sz), variant)
      b = _compress(vol, checker)
      for conn in CONNECTIVITIES:
        for border in BORDERS:
          want = checker.compress(erode_numpy.erode(vol, conn, border), fortran_order=True)
          assert crackle_amd.erode(b, connectivity=conn, erode_border=border) == want, f"{vol.shape} {variant} connectivity={conn} erode_border={border}"
  vol = volumes.edges((sx, 4, 4), variant)
  for conn in CONNECTIVITIES:
    for border in BORDERS:
      _erode_and_check(vol, checker, conn, border)


@pytest.mark.parametrize("kind,shape", volumes.FORMAT_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_row_and_slice_ends_decide_the_crack_format(kind, shape, checker):
  """lib::pixel_pairs < voxels / 2 picks the crack format; the pairs across the ends of rows and slices are part of it
  (tests/test_erode_cpu.py: both formats occur among these cases, and in the first all pairs are of that kind)."""
  vol = volumes.format_case(kind, shape)
  for conn in CONNECTIVITIES:
    expected = erode_numpy.erode(vol, conn, False)
    got = _check(_compress(vol, checker), expected, checker, conn, False)
    assert crackle_amd.header(got).crack_format == (1 if permissible(expected) else 0)


# ---- the border rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", CONNECTIVITIES)
def test_single_label_volume(conn, checker):
  vol = volumes.single_label()
  got = _erode_and_check(vol, checker, conn, True)
  inner = np.zeros(vol.shape, vol.dtype, order="F")
  inner[1:-1, 1:-1, 1:-1] = 7
  assert np.array_equal(crackle_amd.decompress(got), inner)
  b = _compress(vol, checker)
  assert _erode_and_check(vol, checker, conn, False) == b      # unchanged: the stream itself


@pytest.mark.parametrize("shape", [(37, 6, 1), (37, 1, 5), (1, 6, 5), (37, 1, 1), (1, 1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_missing_rows_and_slices_are_ignored_without_the_border_rule(shape, checker):
  vol = volumes.single_label(shape)
  gen = volumes.voronoi((70, 50, 13))[:shape[0], :shape[1], :shape[2]].copy(order="F")
  for conn in CONNECTIVITIES:
    assert _erode_and_check(vol, checker, conn, False) == _compress(vol, checker)
    got = _erode_and_check(vol, checker, conn, True)
    assert got == _compress(np.zeros_like(vol), checker)
    _erode_and_check(gen, checker, conn, False)
    _erode_and_check(gen, checker, conn, True)


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("thickness", [1, 2, 3])
def test_thin_objects(axis, thickness, checker):
  vol = volumes.slab(axis, thickness)
  for conn in CONNECTIVITIES:
    for border in BORDERS:
      got = _erode_and_check(vol, checker, conn, border)
      assert (4 in crackle_amd.labels(got)) == (thickness == 3)


# ---- nothing survives --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", ENCODINGS, ids=ENCODING_IDS)
def test_nothing_survives(kw, checker):
  vol = volumes.thin_sheets()
  zeros = _compress(np.zeros_like(vol), checker)
  for conn in CONNECTIVITIES:
    for border in BORDERS:
      got = _erode_and_check(vol, checker, conn, border, **kw)
      assert got == zeros
      assert crackle_amd.header(got).markov_model_order == 0      # no cracks: compress resets the order
  assert crackle_amd.erode(_compress(vol, checker, **kw), markov_model_order=3) == zeros


def test_stored_width_follows_the_largest_survivor(checker):
  vol = volumes.wide_label_on_a_sheet()
  b = _compress(vol, checker)
  assert crackle_amd.header(b).stored_data_width == 8
  for conn in CONNECTIVITIES:
    for border in BORDERS:
      got = _erode_and_check(vol, checker, conn, border)
      head = crackle_amd.header(got)
      assert head.stored_data_width == 1 and head.data_width == 8
      assert sorted(int(v) for v in crackle_amd.labels(got)) == [0, 3, 4]


# ---- false boundaries --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", CONNECTIVITIES)
def test_false_boundaries_of_remap(conn, checker):
  vol = volumes.merging()
  e = crackle_amd.remap(_compress(vol, checker), volumes.MERGE, preserve_missing_labels=True)
  clean = crackle_amd.recompress(e)
  assert len(clean) < len(e)
  for border in BORDERS:
    got = _check(e, erode_numpy.erode(volumes.merged(vol), conn, border), checker, conn, border)
    assert crackle_amd.erode(clean, connectivity=conn, erode_border=border) == got


@pytest.mark.parametrize("conn", CONNECTIVITIES)
def test_false_boundaries_of_dust_and_fill_holes(conn, checker):
  vol = volumes.merging()
  dusted, removed = dust_numpy.dust(vol, 300, 26)
  assert removed > 0
  e = crackle_amd.dust(_compress(vol, checker), 300, connectivity=26)
  punched = fill_holes_volumes.punched(volumes.GENERATED[0][0], cell=(16, 16, 6))
  filled = fill_holes_numpy.fill_holes(punched, 6)
  assert filled.filled > 0
  f = crackle_amd.fill_holes(_compress(punched, checker), connectivity=6)
  for stream, edited in ((e, np.asfortranarray(dusted)), (f, np.asfortranarray(filled.volume))):
    clean = crackle_amd.recompress(stream)
    assert len(clean) < len(stream)
    for border in BORDERS:
      got = _check(stream, erode_numpy.erode(edited, conn, border), checker, conn, border)
      assert crackle_amd.erode(clean, connectivity=conn, erode_border=border) == got


# ---- widths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.uint64], ids=lambda d: np.dtype(d).name)
def test_every_unsigned_width(dtype, checker):
  vol = volumes.for_dtype(dtype)
  for conn in CONNECTIVITIES:
    for border in BORDERS:
      got = _erode_and_check(vol, checker, conn, border, markov_model_order=2)
      assert crackle_amd.header(got).data_width == np.dtype(dtype).itemsize
  if dtype == np.uint64:
    assert int(crackle_amd.decompress(got).max()) > 1 << 40


def test_labels_that_differ_above_bit_32_are_different(checker):
  vol = volumes.high_bits_only()
  for conn in CONNECTIVITIES:
    for border in BORDERS:
      got = crackle_amd.decompress(_erode_and_check(vol, checker, conn, border))
      assert not got[:, 4:6, :].any() and got[5, 2, 3] == (1 << 32) + 5 and got[5, 7, 3] == (2 << 32) + 5


# ---- both label paths of the encoder -----------------------------------------------------------------------------------
def _encoder_marks(capfd, monkeypatch, stream, conn, border):
  monkeypatch.setenv("CKL_PROFILE", "1")
  capfd.readouterr()
  got = crackle_amd.erode(stream, connectivity=conn, erode_border=border)
  monkeypatch.delenv("CKL_PROFILE", raising=False)
  err = capfd.readouterr().err.splitlines()
  mine = [l for l in err if l.startswith("[ckl erode host ms]")]
  assert len(mine) == 1, err
  fields = dict(w.split("=") for w in mine[0].split()[4:])
  assert list(fields)[:6] == ["tables", "keep_planes", "graph", "cracks", "labels", "assembly"], mine[0]
  assert float(fields["keep_planes"]) > 0 and float(fields["k_erode_device"]) > 0
  enc = [l for l in err if l.startswith("[ckl encode host ms]")]
  return got, sorted(w.split("=")[0] for w in enc[-1].split() if w.startswith("f:"))


def test_strip_path(checker, monkeypatch, capfd):
  vol = volumes.strip_path()
  b = _compress(vol, checker)
  monkeypatch.delenv("CKL_ENC_LABEL_RUNS", raising=False)
  for conn, border in ((26, True), (6, False)):
    got = _check(b, erode_numpy.erode(vol, conn, border), checker, conn, border)
    again, marks = _encoder_marks(capfd, monkeypatch, b, conn, border)
    assert again == got and "f:enqueue_strips" in marks and "f:wait_strips" in marks, marks
    # the same volume with the run pipeline forced
    monkeypatch.setenv("CKL_ENC_LABEL_RUNS", "1")
    again, marks = _encoder_marks(capfd, monkeypatch, b, conn, border)
    monkeypatch.delenv("CKL_ENC_LABEL_RUNS")
    assert again == got and "f:enqueue_runs" in marks and "f:wait_runs" in marks, marks


def test_run_pipeline(checker, monkeypatch, capfd):
  vol = volumes.run_pipeline()
  b = _compress(vol, checker)
  monkeypatch.delenv("CKL_ENC_LABEL_RUNS", raising=False)
  for conn in CONNECTIVITIES:
    got = _check(b, erode_numpy.erode(vol, conn, False), checker, conn, False)
    again, marks = _encoder_marks(capfd, monkeypatch, b, conn, False)
    assert again == got and "f:enqueue_runs" in marks and "f:wait_runs" in marks, marks
  assert _check(b, erode_numpy.erode(vol, 26, True), checker, 26, True) == _compress(np.zeros_like(vol), checker)


# ---- generated ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=volumes.GENERATED, ids=lambda p: "x".join(map(str, p[0])) + p[1])
def generated(request):
  shape, order = request.param
  vol = volumes.voronoi(shape, order)
  assert vol.flags.c_contiguous == (order == "C") and vol.flags.f_contiguous == (order == "F")
  vol.setflags(write=False)
  return vol


@pytest.mark.parametrize("kw", ENCODINGS, ids=ENCODING_IDS)
@pytest.mark.parametrize("border", BORDERS, ids=["erode_border", "keep_border"])
@pytest.mark.parametrize("conn", CONNECTIVITIES)
def test_generated(generated, conn, border, kw, checker):
  b = _compress(generated, checker, **kw)
  head = crackle_amd.header(b)
  assert head.label_format == (2 if kw.get("allow_pins") else 0) and head.fortran_order == bool(generated.flags.f_contiguous)
  got = _check(b, erode_numpy.erode(generated, conn, border), checker, conn, border)
  assert crackle_amd.header(got).markov_model_order == kw.get("markov_model_order", 0)
  assert 2 < crackle_amd.num_labels(got) <= crackle_amd.num_labels(b)


@pytest.mark.parametrize("order", [0, 3])
def test_explicit_markov_order(generated, order, checker):
  b = _compress(generated, checker, markov_model_order=5)
  got = _check(b, erode_numpy.erode(generated, 26, True), checker, 26, True, order=order)
  assert crackle_amd.header(got).markov_model_order == order


@pytest.mark.parametrize("border", BORDERS, ids=["erode_border", "keep_border"])
@pytest.mark.parametrize("conn", CONNECTIVITIES)
def test_two_rounds(generated, conn, border, checker):
  once = erode_numpy.erode(generated, conn, border)
  twice = erode_numpy.erode(once, conn, border)
  assert np.count_nonzero(twice) > 0
  b = _compress(generated, checker)
  first = _check(b, once, checker, conn, border)
  _check(first, twice, checker, conn, border)
  arr = crackle_amd.CrackleArray(b).erode(conn, border).erode(conn, border)
  assert isinstance(arr, crackle_amd.CrackleArray) and arr.binary == checker.compress(twice, fortran_order=bool(generated.flags.f_contiguous))


def test_version_0_stream(checker):
  with np.load(os.path.join(HERE, "golden", "v0.npz")) as z:
    b0 = z[sorted(k for k in z.files if "." not in k)[0]].tobytes()
  head = crackle_amd.header(b0)
  assert head.format_version == 0 and not head.signed
  arr = checker.decompress(b0).reshape((head.sx, head.sy, head.sz), order="F" if head.fortran_order else "C")
  for conn in CONNECTIVITIES:
    for border in BORDERS:
      _check(b0, erode_numpy.erode(arr, conn, border), checker, conn, border)


def test_repeatable(checker):
  vol = volumes.merging()
  b = _compress(vol, checker, markov_model_order=4)
  outs = [crackle_amd.erode(b) for _ in range(3)]
  assert outs[0] == outs[1] == outs[2] == checker.compress(erode_numpy.erode(vol), markov_model_order=4)


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_errors_on_the_device_side(checker):
  lab = volumes.voronoi((48, 40, 5), dtype=np.uint16, cell=(8, 8, 2))
  b = _compress(lab, checker)
  # a damaged slice: what decompress raises for it
  head = crackle_amd.header(b)
  lens = [int.from_bytes(b[29 + 4 * z:33 + 4 * z], "little") for z in range(head.sz)]
  codes = head.header_bytes + head.grid_index_bytes + head.num_label_bytes
  bad = bytearray(b)
  bad[codes + lens[0] + lens[1] + lens[2] // 2] ^= 0xFF
  with pytest.raises(Exception) as seen:
    crackle_amd.decompress(bytes(bad))
  assert "z=2" in str(seen.value)
  for conn in CONNECTIVITIES:
    with pytest.raises(type(seen.value), match=re.escape(str(seen.value))):
      crackle_amd.erode(bytes(bad), connectivity=conn)
  assert crackle_amd.erode(b) == checker.compress(erode_numpy.erode(lab))      # the session pool is none the worse for it
