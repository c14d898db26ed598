"""GPU tests of crackle_amd.downsample (ckl_downsample: the decoder's run tables -> k_erode_run_labels, k_pool_cuts,
k_pool_labels, k_pool_planes -> the encoder's crack and label stages for the POOLED shape; crackle_amd/csrc/ckl_downsample.hpp
and ckl_recompress.hip).

The check throughout: downsample(stream, f)[0] equals the checker's compress of the restated pooling
(tests/downsample_numpy.py, worked from the INPUT array) byte for byte under the requested markov order (default: the
stream's); the result decodes, here and with the checker, to that array in the input's dtype and memory order;
crackle_amd.ok() accepts it; its labels are the array's; its header is FLAT, version 1, with the input's data width and
order flag.  The volumes and what each of them is about: tests/downsample_volumes.py, pinned on the CPU by
tests/test_downsample_cpu.py."""
import os
import re

import numpy as np
import pytest

import crackle_amd
import downsample_numpy
import downsample_volumes as volumes
import dust_numpy
import erode_volumes
import stream_kinds
from recompress_volumes import permissible
from crackle_amd import downsample      # (the feature under test: without it nothing here runs)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FACTORS = volumes.FACTORS
FACTOR_IDS = ["2x2x1", "2x2x2"]
ENCODINGS = [dict(), dict(allow_pins=True), dict(markov_model_order=5)]
ENCODING_IDS = ["flat", "pins", "markov5"]


def _compress(vol, checker, **kw):
  return checker.compress(vol, fortran_order=bool(vol.flags.f_contiguous), **kw)


def _check(stream, expected, checker, factor, order=None):
  """expected: the restated pooling, in the memory order of the stream's flag."""
  head = crackle_amd.header(stream)
  m = head.markov_model_order if order is None else order
  want = checker.compress(expected, fortran_order=head.fortran_order, markov_model_order=m)
  levels = crackle_amd.downsample(stream, factor, markov_model_order=order)
  assert isinstance(levels, list) and len(levels) == 1
  got = levels[0]
  assert got == want, f"{expected.shape} {expected.dtype} factor={factor} order={order}"
  out = crackle_amd.header(got)
  assert out.label_format == 0 and out.format_version == 1 and out.data_width == head.data_width and out.fortran_order == head.fortran_order
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


def _pool_and_check(vol, checker, factor, order=None, **kw):
  return _check(_compress(vol, checker, **kw), downsample_numpy.downsample(vol, factor), checker, factor, order=order)


# ---- word and row edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", volumes.EDGE_VARIANTS)
@pytest.mark.parametrize("sx", volumes.EDGE_SX)
def test_word_and_row_edges(sx, variant, checker):
  """Every sy, sz of 1 .. 4 at both factors, byte for byte; all of the checks on the largest."""
  for sy in volumes.EDGE_SYZ:
    for sz in volumes.EDGE_SYZ:
      vol = volumes.edges((sx, sy, sz), variant)
      b = _compress(vol, checker)
      for factor in FACTORS:
        want = checker.compress(downsample_numpy.downsample(vol, factor), fortran_order=True)
        assert crackle_amd.downsample(b, factor) == [want], f"{vol.shape} {variant} factor={factor}"
  for shape in ((sx, 4, 4), (sx, 3, 3)):
    for factor in FACTORS:
      _pool_and_check(volumes.edges(shape, variant), checker, factor)


# ---- hand-built blocks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype,values,answer", volumes.BLOCKS_221, ids=[c[0] for c in volumes.BLOCKS_221])
def test_reference_rule(name, dtype, values, answer, checker):
  blk = volumes.block(dtype, values, (2, 2, 1))
  for x0 in volumes.PLACES:
    got = _pool_and_check(volumes.place(blk, x0), checker, (2, 2, 1))
    assert int(crackle_amd.decompress(got)[x0 // 2, 1, 0]) == answer      # (the literal answer)


@pytest.mark.parametrize("name,dtype,values,answer", volumes.BLOCKS_222, ids=[c[0] for c in volumes.BLOCKS_222])
def test_mode_and_tie_rule(name, dtype, values, answer, checker):
  blk = volumes.block(dtype, values)
  for x0 in volumes.PLACES:
    got = _pool_and_check(volumes.place(blk, x0), checker, (2, 2, 2))
    assert int(crackle_amd.decompress(got)[x0 // 2, 1, 0]) == answer      # (the literal answer)


@pytest.mark.parametrize("name,shape,values,per_slice,mode", volumes.PARTIAL, ids=[c[0] for c in volumes.PARTIAL])
def test_partial_blocks(name, shape, values, per_slice, mode, checker):
  blk = volumes.block(np.uint8, values, shape)
  for x0 in volumes.PLACES:
    vol = volumes.place(blk, x0)
    got = _pool_and_check(vol, checker, (2, 2, 1))
    assert crackle_amd.decompress(got)[x0 // 2, 1, :].tolist() == list(per_slice)
    got = _pool_and_check(vol, checker, (2, 2, 2))
    assert int(crackle_amd.decompress(got)[x0 // 2, 1, 0]) == mode
  for factor in FACTORS:
    _pool_and_check(blk, checker, factor)      # the block alone: volumes of one to four voxels


# ---- the crack format --------------------------------------------------------------------------------------------------
def test_mixed_formats(checker):
  """mode_pooling_2x2x1 cannot stack the pooled slices of this volume; downsample encodes the pooled volume as a whole."""
  vol = volumes.mixed_formats()
  b = _compress(vol, checker)
  with pytest.raises(ValueError, match="crack format"):
    crackle_amd.mode_pooling_2x2x1(b)
  _pool_and_check(vol, checker, (2, 2, 1))
  _pool_and_check(vol, checker, (2, 2, 2))


@pytest.mark.parametrize("name,pattern,before,after", volumes.FORMAT_CASES, ids=[c[0] for c in volumes.FORMAT_CASES])
def test_the_crack_format_follows_the_pooled_volume(name, pattern, before, after, checker):
  vol = volumes.rows(pattern)
  b = _compress(vol, checker)
  assert crackle_amd.header(b).crack_format == (1 if before else 0) and permissible(vol) == before
  for factor in FACTORS:
    expected = downsample_numpy.downsample(vol, factor)
    got = _check(b, expected, checker, factor)
    assert permissible(expected) == after and crackle_amd.header(got).crack_format == (1 if after else 0)


# ---- labels that vanish ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", FACTORS, ids=FACTOR_IDS)
def test_lonely_labels_vanish(factor, checker):
  vol = volumes.lonely_labels()
  b = _compress(vol, checker)
  assert crackle_amd.num_labels(b) > 301
  got = _check(b, downsample_numpy.downsample(vol, factor), checker, factor)
  assert crackle_amd.labels(got).tolist() == [5]      # the largest input label is among the losers
  assert len(got) < len(b)


@pytest.mark.parametrize("n", (255, 256, 257))
def test_survivors_around_a_byte_of_index(n, checker):
  vol = volumes.survivors(n)
  b = _compress(vol, checker)
  assert crackle_amd.num_labels(b) > n
  for factor in FACTORS:
    got = _check(b, downsample_numpy.downsample(vol, factor), checker, factor)
    assert crackle_amd.num_labels(got) == n


# ---- generated ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=range(len(volumes.GENERATED)), ids=["x".join(map(str, g[0])) + g[1] for g in volumes.GENERATED])
def generated(request):
  vol = volumes.generated(request.param)
  vol.setflags(write=False)
  return vol


@pytest.mark.parametrize("kw", ENCODINGS, ids=ENCODING_IDS)
@pytest.mark.parametrize("factor", FACTORS, ids=FACTOR_IDS)
def test_generated(generated, factor, kw, checker):
  b = _compress(generated, checker, **kw)
  head = crackle_amd.header(b)
  assert head.label_format == (2 if kw.get("allow_pins") else 0) and head.fortran_order == bool(generated.flags.f_contiguous)
  got = _check(b, downsample_numpy.downsample(generated, factor), checker, factor)
  assert crackle_amd.header(got).markov_model_order == kw.get("markov_model_order", 0)
  if factor == (2, 2, 1) and not kw:
    assert np.array_equal(crackle_amd.decompress(got), crackle_amd.decompress(crackle_amd.mode_pooling_2x2x1(b)))


@pytest.mark.parametrize("order", [0, 3])
def test_explicit_markov_order(generated, order, checker):
  b = _compress(generated, checker, markov_model_order=5)
  for factor in FACTORS:
    got = _check(b, downsample_numpy.downsample(generated, factor), checker, factor, order=order)
    assert crackle_amd.header(got).markov_model_order == order


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.uint64], ids=lambda d: np.dtype(d).name)
def test_every_unsigned_width(dtype, checker):
  vol = volumes.for_dtype(dtype)
  for factor in FACTORS:
    got = _pool_and_check(vol, checker, factor, markov_model_order=2)
    assert crackle_amd.header(got).data_width == np.dtype(dtype).itemsize
    if dtype == np.uint64:
      assert int(crackle_amd.decompress(got).max()) > 1 << 40


@pytest.mark.parametrize("factor", FACTORS, ids=FACTOR_IDS)
def test_many_workgroups_of_words(factor, checker):
  _pool_and_check(volumes.voronoi(volumes.MANY_WORDS), checker, factor)


@pytest.mark.parametrize("shape", [(37, 1, 1), (1, 6, 5), (1, 1, 1), (2, 2, 2), (64, 2, 2), (65, 2, 1)], ids=lambda s: "x".join(map(str, s)))
def test_missing_rows_and_slices(shape, checker):
  vol = volumes.generated(0)[:shape[0], :shape[1], :shape[2]].copy(order="F")
  for factor in FACTORS:
    _pool_and_check(vol, checker, factor)


# ---- both label paths of the encoder, and the profile line -------------------------------------------------------------
def _profiled(capfd, monkeypatch, stream, factor):
  monkeypatch.setenv("CKL_PROFILE", "1")
  capfd.readouterr()
  got = crackle_amd.downsample(stream, factor)[0]
  monkeypatch.delenv("CKL_PROFILE", raising=False)
  err = capfd.readouterr().err.splitlines()
  mine = [l for l in err if l.startswith("[ckl downsample host ms]")]
  assert len(mine) == 1, err
  fields = dict(w.split("=") for w in mine[0].split()[4:])
  assert list(fields) == ["tables", "pool_planes", "graph", "cracks", "labels", "assembly", "k_pool_device", "pieces"], mine[0]
  assert float(fields["pool_planes"]) > 0 and float(fields["k_pool_device"]) > 0
  enc = [l for l in err if l.startswith("[ckl encode host ms]")]
  return got, sorted(w.split("=")[0] for w in enc[-1].split() if w.startswith("f:")), int(fields["pieces"])


def test_strip_path(checker, monkeypatch, capfd):
  vol = volumes.strip_path()
  b = _compress(vol, checker)
  monkeypatch.delenv("CKL_ENC_LABEL_RUNS", raising=False)
  for factor in FACTORS:
    expected = downsample_numpy.downsample(vol, factor)
    got = _check(b, expected, checker, factor)
    again, marks, pieces = _profiled(capfd, monkeypatch, b, factor)
    assert again == got and "f:enqueue_strips" in marks and "f:wait_strips" in marks, marks
    assert pieces == downsample_numpy.pooled_runs(expected)
    if factor == (2, 2, 1):
      # the same volume with the run pipeline forced
      monkeypatch.setenv("CKL_ENC_LABEL_RUNS", "1")
      again, marks, pieces = _profiled(capfd, monkeypatch, b, factor)
      monkeypatch.delenv("CKL_ENC_LABEL_RUNS")
      assert again == got and "f:enqueue_runs" in marks and "f:wait_runs" in marks, marks
      assert pieces == downsample_numpy.pooled_runs(expected)


def test_run_pipeline(checker, monkeypatch, capfd):
  vol = volumes.run_pipeline()
  b = _compress(vol, checker)
  monkeypatch.delenv("CKL_ENC_LABEL_RUNS", raising=False)
  expected = downsample_numpy.downsample(vol, (2, 2, 1))
  got = _check(b, expected, checker, (2, 2, 1))
  again, marks, pieces = _profiled(capfd, monkeypatch, b, (2, 2, 1))
  assert again == got and "f:enqueue_runs" in marks and "f:wait_runs" in marks, marks
  assert pieces == downsample_numpy.pooled_runs(expected)


@pytest.mark.parametrize("factor", FACTORS, ids=FACTOR_IDS)
def test_profile_line(factor, generated, checker, monkeypatch, capfd):
  b = _compress(generated, checker)
  expected = downsample_numpy.downsample(generated, factor)
  got, _, pieces = _profiled(capfd, monkeypatch, b, factor)
  assert got == checker.compress(expected, fortran_order=bool(generated.flags.f_contiguous))
  assert pieces == downsample_numpy.pooled_runs(expected) > expected.shape[1] * expected.shape[2]


# ---- false boundaries --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", FACTORS, ids=FACTOR_IDS)
def test_false_boundaries_of_remap(factor, checker):
  vol = erode_volumes.merging()
  e = crackle_amd.remap(_compress(vol, checker), erode_volumes.MERGE, preserve_missing_labels=True)
  clean = crackle_amd.recompress(e)
  assert len(clean) < len(e)
  got = _check(e, downsample_numpy.downsample(erode_volumes.merged(vol), factor), checker, factor)
  assert crackle_amd.downsample(clean, factor) == [got]


@pytest.mark.parametrize("factor", FACTORS, ids=FACTOR_IDS)
def test_false_boundaries_of_dust(factor, checker):
  vol = erode_volumes.merging()
  dusted, removed = dust_numpy.dust(vol, 300, 26)
  assert removed > 0
  e = crackle_amd.dust(_compress(vol, checker), 300, connectivity=26)
  clean = crackle_amd.recompress(e)
  assert len(clean) < len(e)
  got = _check(e, downsample_numpy.downsample(np.asfortranarray(dusted), factor), checker, factor)
  assert crackle_amd.downsample(clean, factor) == [got]


# ---- every kind of stream ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kinds(checker):
  vol = stream_kinds.volume_a()
  return {k.name: k for k in stream_kinds.kinds_host(vol, checker) + stream_kinds.kinds_device(vol, checker)}


@pytest.mark.parametrize("name", stream_kinds.HOST_KINDS + stream_kinds.DEVICE_KINDS)
def test_every_stream_kind(name, kinds, checker):
  kind = kinds[name]
  for factor in FACTORS:
    _check(kind.stream, downsample_numpy.downsample(kind.expected, factor), checker, factor)


def test_version_0_stream(checker):
  with np.load(os.path.join(HERE, "golden", "v0.npz")) as z:
    b0 = z[sorted(k for k in z.files if "." not in k)[0]].tobytes()
  head = crackle_amd.header(b0)
  assert head.format_version == 0 and not head.signed
  arr = checker.decompress(b0).reshape((head.sx, head.sy, head.sz), order="F" if head.fortran_order else "C")
  for factor in FACTORS:
    _check(b0, downsample_numpy.downsample(arr, factor), checker, factor)


# ---- the pyramid -------------------------------------------------------------------------------------------------------
def test_pyramid(checker):
  vol = volumes.generated(1)
  assert vol.shape == (97, 61, 12)
  b = _compress(vol, checker, markov_model_order=2)
  levels = crackle_amd.downsample(b, (2, 2, 2), num_mips=4)
  want = downsample_numpy.pyramid(vol, (2, 2, 2), 4)
  assert [w.shape for w in want] == [(49, 31, 6), (25, 16, 3), (13, 8, 2), (7, 4, 1)]
  assert len(levels) == 4
  for got, expected in zip(levels, want):
    assert got == checker.compress(expected, fortran_order=False, markov_model_order=2)
    head = crackle_amd.header(got)
    assert (head.sx, head.sy, head.sz) == expected.shape
  assert [a.binary for a in crackle_amd.CrackleArray(b).downsample((2, 2, 2), 4)] == levels
  flat = crackle_amd.downsample(b, (2, 2, 1), num_mips=3, markov_model_order=0)
  assert flat == [checker.compress(w, fortran_order=False) for w in downsample_numpy.pyramid(vol, (2, 2, 1), 3)]
  one = np.full((1, 1, 1), 77, np.uint32, order="F")
  for factor in FACTORS:
    assert crackle_amd.downsample(_compress(one, checker), factor, num_mips=3) == [_compress(one, checker)] * 3


# ---- repeatability and damage ------------------------------------------------------------------------------------------
def test_repeatable(checker):
  vol = volumes.voronoi(volumes.MANY_WORDS)
  b = _compress(vol, checker, markov_model_order=4)
  for factor in FACTORS:
    outs = [crackle_amd.downsample(b, factor)[0] for _ in range(3)]
    assert outs[0] == outs[1] == outs[2] == checker.compress(downsample_numpy.downsample(vol, factor), markov_model_order=4)


def test_errors_on_the_device_side(checker):
  lab = erode_volumes.voronoi((48, 40, 5), dtype=np.uint16, cell=(8, 8, 2))
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
  for factor in FACTORS:
    with pytest.raises(type(seen.value), match=re.escape(str(seen.value))):
      crackle_amd.downsample(bytes(bad), factor)
    assert crackle_amd.downsample(b, factor) == [checker.compress(downsample_numpy.downsample(lab, factor))]      # the session pool is none the worse for it
