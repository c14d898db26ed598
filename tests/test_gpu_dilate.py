"""GPU tests of crackle_amd.dilate (ckl_dilate: the decoder's run tables -> k_erode_run_labels, k_dilate_nonzero,
k_dilate_gain, k_dilate_mode, k_dilate_planes -> the encoder's crack and label stages; crackle_amd/csrc/ckl_dilate.hpp
and ckl_recompress.hip), and of opening and closing on top of it.

The check throughout: dilate(stream, ...) equals the checker's compress of the restated dilation (tests/dilate_numpy.py,
worked from the INPUT array) byte for byte under the requested markov order (default: the stream's); the result
decodes, here and with the checker, to that array in the input's dtype and memory order; crackle_amd.ok() accepts it;
its labels are the array's; its header is FLAT, version 1, with the input's data width and order flag.  The volumes
and what each of them is about: tests/dilate_volumes.py, pinned on the CPU by tests/test_dilate_cpu.py."""
import os
import re

import numpy as np
import pytest

import crackle_amd
import dilate_numpy
import dilate_volumes as volumes
import dust_numpy
import erode_numpy
import erode_volumes
import stream_kinds
from recompress_volumes import permissible
from crackle_amd import dilate      # (the feature under test: without it nothing here runs)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CONNECTIVITIES = volumes.CONNECTIVITIES
ENCODINGS = [dict(), dict(allow_pins=True), dict(markov_model_order=5)]
ENCODING_IDS = ["flat", "pins", "markov5"]


def _compress(vol, checker, **kw):
  return checker.compress(vol, fortran_order=bool(vol.flags.f_contiguous), **kw)


def _check(stream, expected, checker, conn, order=None):
  """expected: the restated dilation, in the memory order of the stream's flag."""
  head = crackle_amd.header(stream)
  m = head.markov_model_order if order is None else order
  want = checker.compress(expected, fortran_order=head.fortran_order, markov_model_order=m)
  got = crackle_amd.dilate(stream, connectivity=conn, markov_model_order=order)
  assert got == want, f"{expected.shape} {expected.dtype} connectivity={conn} order={order}"
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


def _dilate_and_check(vol, checker, conn, order=None, **kw):
  return _check(_compress(vol, checker, **kw), dilate_numpy.dilate(vol, conn), checker, conn, order=order)


# ---- which neighbour counts --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", volumes.NEIGHBOURS, ids=lambda o: "%+d%+d%+d" % o)
def test_which_neighbour_counts(offset, checker):
  vol = volumes.probe(offset)
  b = _compress(vol, checker)
  for conn in CONNECTIVITIES:
    got = _check(b, dilate_numpy.dilate(vol, conn), checker, conn)
    centre = crackle_amd.decompress(got)[volumes.PROBE_CENTRE]
    assert (centre == 3) == volumes.probe_centre_gained(offset, conn)      # (stated literally there)
    assert centre in (0, 3)


# ---- the mode and the tie rule -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype,entries,answers", volumes.MODE_CASES, ids=[c[0] for c in volumes.MODE_CASES])
def test_mode_and_tie_rule(name, dtype, entries, answers, checker):
  vol = volumes.mode_case(dtype, entries)
  for conn, answer in zip(CONNECTIVITIES, answers):
    got = _dilate_and_check(vol, checker, conn)
    assert int(crackle_amd.decompress(got)[volumes.MODE_CENTRE]) == answer      # (the literal answer)


# ---- word and row edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", volumes.EDGE_VARIANTS)
@pytest.mark.parametrize("sx", volumes.EDGE_SX)
def test_word_and_row_edges(sx, variant, checker):
  """Every sy, sz of 1 .. 4 at every connectivity, byte for byte; all of the checks on the largest."""
  for sy in volumes.EDGE_SYZ:
    for sz in volumes.EDGE_SYZ:
      vol = volumes.edges((sx, sy, sz), variant)
      b = _compress(vol, checker)
      for conn in CONNECTIVITIES:
        want = checker.compress(dilate_numpy.dilate(vol, conn), fortran_order=True)
        assert crackle_amd.dilate(b, connectivity=conn) == want, f"{vol.shape} {variant} connectivity={conn}"
  vol = volumes.edges((sx, 4, 4), variant)
  for conn in CONNECTIVITIES:
    _dilate_and_check(vol, checker, conn)


@pytest.mark.parametrize("name,pattern", volumes.FORMAT_CASES, ids=[c[0] for c in volumes.FORMAT_CASES])
def test_the_crack_format_follows_the_dilated_volume(name, pattern, checker):
  """lib::pixel_pairs < voxels / 2 picks the crack format; here all pairs are wrap-arounds (tests/test_dilate_cpu.py:
  the first case is PERMISSIBLE before and IMPERMISSIBLE after, the second stays PERMISSIBLE)."""
  vol = volumes.rows(pattern)
  b = _compress(vol, checker)
  assert crackle_amd.header(b).crack_format == 1 and permissible(vol)
  for conn in CONNECTIVITIES:
    expected = dilate_numpy.dilate(vol, conn)
    got = _check(b, expected, checker, conn)
    assert crackle_amd.header(got).crack_format == (1 if permissible(expected) else 0)
    assert permissible(expected) == (name != "1-0-2-0")


# ---- nothing gained ----------------------------------------------------------------------------------------------------
def test_nothing_gained(checker):
  vol = volumes.no_background()
  b = _compress(vol, checker, markov_model_order=2)
  zeros = np.zeros((37, 6, 5), np.uint16, order="F")
  bz = _compress(zeros, checker)
  for conn in CONNECTIVITIES:
    assert _check(b, vol, checker, conn) == crackle_amd.recompress(b) == b
    assert _check(bz, zeros, checker, conn) == bz
  pins = _compress(vol, checker, allow_pins=True)
  assert crackle_amd.dilate(pins) == crackle_amd.recompress(pins) == _compress(vol, checker)


@pytest.mark.parametrize("conn", CONNECTIVITIES)
def test_single_voxel(conn, checker):
  vol = volumes.single_voxel()
  got = _dilate_and_check(vol, checker, conn)
  out = crackle_amd.decompress(got)
  assert int(np.count_nonzero(out)) == 1 + conn and set(np.unique(out).tolist()) == {0, 7}


@pytest.mark.parametrize("shape", [(37, 1, 1), (1, 6, 5), (1, 1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_missing_rows_and_slices(shape, checker):
  gen = volumes.seams((70, 50, 13))[:shape[0], :shape[1], :shape[2]].copy(order="F")
  alternating = np.zeros(shape, np.uint8, order="F")
  alternating.reshape(-1, order="F")[::3] = 1 + np.arange(len(alternating.reshape(-1, order="F")[::3])) % 5
  for conn in CONNECTIVITIES:
    _dilate_and_check(gen, checker, conn)
    _dilate_and_check(alternating, checker, conn)


# ---- generated ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", CONNECTIVITIES)
def test_many_workgroups_of_words(conn, checker):
  vol = volumes.seams(volumes.MANY_WORDS)
  _dilate_and_check(vol, checker, conn)


@pytest.fixture(scope="module", params=volumes.GENERATED, ids=lambda p: "x".join(map(str, p[0])) + p[1])
def generated(request):
  shape, order = request.param
  vol = volumes.seams(shape, order)
  assert vol.flags.c_contiguous == (order == "C") and vol.flags.f_contiguous == (order == "F")
  vol.setflags(write=False)
  return vol


@pytest.mark.parametrize("kw", ENCODINGS, ids=ENCODING_IDS)
@pytest.mark.parametrize("conn", CONNECTIVITIES)
def test_generated(generated, conn, kw, checker):
  b = _compress(generated, checker, **kw)
  head = crackle_amd.header(b)
  assert head.label_format == (2 if kw.get("allow_pins") else 0) and head.fortran_order == bool(generated.flags.f_contiguous)
  got = _check(b, dilate_numpy.dilate(generated, conn), checker, conn)
  assert crackle_amd.header(got).markov_model_order == kw.get("markov_model_order", 0)
  assert crackle_amd.num_labels(got) == crackle_amd.num_labels(b) > 2      # background is left, no label appears or goes


@pytest.mark.parametrize("order", [0, 3])
def test_explicit_markov_order(generated, order, checker):
  b = _compress(generated, checker, markov_model_order=5)
  got = _check(b, dilate_numpy.dilate(generated, 26), checker, 26, order=order)
  assert crackle_amd.header(got).markov_model_order == order


@pytest.mark.parametrize("conn", CONNECTIVITIES)
def test_two_rounds(generated, conn, checker):
  once = dilate_numpy.dilate(generated, conn)
  twice = dilate_numpy.dilate(once, conn)
  assert np.count_nonzero(twice) > np.count_nonzero(once) > np.count_nonzero(generated)
  b = _compress(generated, checker)
  first = _check(b, once, checker, conn)
  _check(first, twice, checker, conn)
  arr = crackle_amd.CrackleArray(b).dilate(conn).dilate(conn)
  assert isinstance(arr, crackle_amd.CrackleArray) and arr.binary == checker.compress(twice, fortran_order=bool(generated.flags.f_contiguous))


# ---- widths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.uint64], ids=lambda d: np.dtype(d).name)
def test_every_unsigned_width(dtype, checker):
  vol = volumes.for_dtype(dtype)
  for conn in CONNECTIVITIES:
    got = _dilate_and_check(vol, checker, conn, markov_model_order=2)
    assert crackle_amd.header(got).data_width == np.dtype(dtype).itemsize
  if dtype == np.uint64:
    out = crackle_amd.decompress(got)
    assert int(out[(vol == 0) & (out != 0)].min()) > 1 << 40      # gained labels above 2^40


# ---- both label paths of the encoder -----------------------------------------------------------------------------------
def _encoder_marks(capfd, monkeypatch, stream, conn):
  monkeypatch.setenv("CKL_PROFILE", "1")
  capfd.readouterr()
  got = crackle_amd.dilate(stream, connectivity=conn)
  monkeypatch.delenv("CKL_PROFILE", raising=False)
  err = capfd.readouterr().err.splitlines()
  mine = [l for l in err if l.startswith("[ckl dilate host ms]")]
  assert len(mine) == 1, err
  fields = dict(w.split("=") for w in mine[0].split()[4:])
  assert list(fields) == ["tables", "gain_planes", "graph", "cracks", "labels", "assembly", "k_dilate_device", "gained"], mine[0]
  assert float(fields["gain_planes"]) > 0 and float(fields["k_dilate_device"]) > 0
  enc = [l for l in err if l.startswith("[ckl encode host ms]")]
  return got, sorted(w.split("=")[0] for w in enc[-1].split() if w.startswith("f:")), int(fields["gained"])


def _gained(vol, conn):
  return int(np.count_nonzero(vol == 0) - np.count_nonzero(dilate_numpy.dilate(vol, conn) == 0))


def test_strip_path(checker, monkeypatch, capfd):
  vol = volumes.strip_path()
  b = _compress(vol, checker)
  monkeypatch.delenv("CKL_ENC_LABEL_RUNS", raising=False)
  for conn in (26, 6):
    got = _check(b, dilate_numpy.dilate(vol, conn), checker, conn)
    again, marks, gained = _encoder_marks(capfd, monkeypatch, b, conn)
    assert again == got and "f:enqueue_strips" in marks and "f:wait_strips" in marks, marks
    assert gained == _gained(vol, conn) > 0
    # the same volume with the run pipeline forced
    monkeypatch.setenv("CKL_ENC_LABEL_RUNS", "1")
    again, marks, gained = _encoder_marks(capfd, monkeypatch, b, conn)
    monkeypatch.delenv("CKL_ENC_LABEL_RUNS")
    assert again == got and "f:enqueue_runs" in marks and "f:wait_runs" in marks, marks
    assert gained == _gained(vol, conn)


def test_run_pipeline(checker, monkeypatch, capfd):
  vol = volumes.run_pipeline()
  b = _compress(vol, checker)
  monkeypatch.delenv("CKL_ENC_LABEL_RUNS", raising=False)
  for conn in CONNECTIVITIES:
    got = _check(b, dilate_numpy.dilate(vol, conn), checker, conn)
    again, marks, gained = _encoder_marks(capfd, monkeypatch, b, conn)
    assert again == got and "f:enqueue_runs" in marks and "f:wait_runs" in marks, marks
    assert gained == _gained(vol, conn) > 0


def test_profile_line_of_a_stream_that_gains_nothing(checker, monkeypatch, capfd):
  b = _compress(volumes.no_background((40, 30, 4)), checker)
  got, _, gained = _encoder_marks(capfd, monkeypatch, b, 26)
  assert got == b and gained == 0


# ---- false boundaries --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", CONNECTIVITIES)
def test_false_boundaries_of_remap(conn, checker):
  vol = erode_volumes.merging()
  e = crackle_amd.remap(_compress(vol, checker), erode_volumes.MERGE, preserve_missing_labels=True)
  clean = crackle_amd.recompress(e)
  assert len(clean) < len(e)
  got = _check(e, dilate_numpy.dilate(erode_volumes.merged(vol), conn), checker, conn)
  assert crackle_amd.dilate(clean, connectivity=conn) == got


@pytest.mark.parametrize("conn", CONNECTIVITIES)
def test_false_boundaries_of_dust(conn, checker):
  vol = erode_volumes.merging()
  dusted, removed = dust_numpy.dust(vol, 300, 26)
  assert removed > 0
  e = crackle_amd.dust(_compress(vol, checker), 300, connectivity=26)
  clean = crackle_amd.recompress(e)
  assert len(clean) < len(e)
  got = _check(e, dilate_numpy.dilate(np.asfortranarray(dusted), conn), checker, conn)
  assert crackle_amd.dilate(clean, connectivity=conn) == got


# ---- every kind of stream ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kinds(checker):
  vol = stream_kinds.volume_a()
  return {k.name: k for k in stream_kinds.kinds_host(vol, checker) + stream_kinds.kinds_device(vol, checker)}


@pytest.mark.parametrize("name", stream_kinds.HOST_KINDS + stream_kinds.DEVICE_KINDS)
def test_every_stream_kind(name, kinds, checker):
  kind = kinds[name]
  assert (np.asarray(kind.expected) == 0).any()
  for conn in CONNECTIVITIES:
    expected = dilate_numpy.dilate(kind.expected, conn)
    assert not np.array_equal(expected, kind.expected)
    _check(kind.stream, expected, checker, conn)


def test_version_0_stream(checker):
  with np.load(os.path.join(HERE, "golden", "v0.npz")) as z:
    b0 = z[sorted(k for k in z.files if "." not in k)[0]].tobytes()
  head = crackle_amd.header(b0)
  assert head.format_version == 0 and not head.signed
  arr = checker.decompress(b0).reshape((head.sx, head.sy, head.sz), order="F" if head.fortran_order else "C")
  for conn in CONNECTIVITIES:
    _check(b0, dilate_numpy.dilate(arr, conn), checker, conn)


def test_repeatable(checker):
  vol = volumes.seams(volumes.MANY_WORDS)
  b = _compress(vol, checker, markov_model_order=4)
  outs = [crackle_amd.dilate(b) for _ in range(3)]
  assert outs[0] == outs[1] == outs[2] == checker.compress(dilate_numpy.dilate(vol), markov_model_order=4)


# ---- opening and closing -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", (True, False), ids=["erode_border", "keep_border"])
@pytest.mark.parametrize("conn", CONNECTIVITIES)
def test_opening_and_closing(generated, conn, border, checker):
  b = _compress(generated, checker, markov_model_order=4)
  f = bool(generated.flags.f_contiguous)
  opened = dilate_numpy.dilate(erode_numpy.erode(generated, conn, border), conn)
  closed = erode_numpy.erode(dilate_numpy.dilate(generated, conn), conn, border)
  assert opened.any() and closed.any() and not np.array_equal(opened, closed)
  assert crackle_amd.opening(b, conn, border) == checker.compress(opened, fortran_order=f, markov_model_order=4)
  assert crackle_amd.closing(b, conn, border) == checker.compress(closed, fortran_order=f, markov_model_order=4)
  assert crackle_amd.opening(b, conn, border, markov_model_order=0) == checker.compress(opened, fortran_order=f)
  assert crackle_amd.closing(b, conn, border, markov_model_order=2) == checker.compress(closed, fortran_order=f, markov_model_order=2)
  arr = crackle_amd.CrackleArray(b)
  assert arr.opening(conn, border).binary == crackle_amd.opening(b, conn, border) and arr.closing(conn, border).binary == crackle_amd.closing(b, conn, border)


@pytest.mark.parametrize("conn", CONNECTIVITIES)
def test_closing_fills_a_pit(conn, checker):
  vol = volumes.pit()
  out = crackle_amd.decompress(crackle_amd.closing(_compress(vol, checker), conn))
  assert np.array_equal(out, erode_numpy.erode(dilate_numpy.dilate(vol, conn), conn, True))
  assert out[8, 5, 4] == 6 and (out[10, 5, 6] == 6) == (conn != 6)      # (tests/dilate_volumes.py: pit)
  assert np.array_equal(out != 0, (vol != 0) | (out != vol)) and int(np.count_nonzero(out != vol)) == (1 if conn == 6 else 2)


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_errors_on_the_device_side(checker):
  lab = volumes.seams((48, 40, 5), dtype=np.uint16, cell=(8, 8, 2))
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
      crackle_amd.dilate(bytes(bad), connectivity=conn)
  assert crackle_amd.dilate(b) == checker.compress(dilate_numpy.dilate(lab))      # the session pool is none the worse for it
