"""GPU tests of crackle_amd.overlay and crackle_amd.mask_by (ckl_combine: two decode sessions' run tables ->
k_erode_run_labels twice, k_combine_cuts, k_combine_labels, k_pool_planes -> the encoder's crack and label stages;
crackle_amd/csrc/ckl_combine.hpp and ckl_recompress.hip).

The check throughout, for the three rules: the result equals the checker's compress of the restated combination
(tests/combine_numpy.py, worked from the two INPUT arrays) byte for byte under the requested markov order (default: the
first stream's) and the first stream's order flag; it decodes, here and with the checker, to that array in the right dtype
and memory order; crackle_amd.ok() accepts it; its labels are the array's; its header is FLAT, version 1, with the data
width of the restated array.  The pairs and what each of them is about: tests/combine_volumes.py, pinned on the CPU by
tests/test_combine_cpu.py."""
import os
import re

import numpy as np
import pytest

import crackle_amd
import combine_numpy
import combine_volumes as volumes
import dust_numpy
import erode_volumes
import stream_kinds
from recompress_volumes import permissible
from crackle_amd import overlay, mask_by      # (the feature under test: without it nothing here runs)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RULES = combine_numpy.RULES
ENCODINGS = [dict(), dict(allow_pins=True), dict(markov_model_order=5)]
ENCODING_IDS = ["flat", "pins", "markov5"]


def _compress(vol, checker, **kw):
  return checker.compress(vol, fortran_order=bool(vol.flags.f_contiguous), **kw)


def _call(rule, a, b, **kw):
  if rule == "overlay":
    return overlay(a, b, **kw)
  return mask_by(a, b, invert=(rule == "drop"), **kw)


def _check(stream_a, stream_b, expected, checker, rule, order=None):
  """expected: the restated combination, in the memory order of the first stream's flag."""
  head = crackle_amd.header(stream_a)
  m = head.markov_model_order if order is None else order
  want = checker.compress(expected, fortran_order=head.fortran_order, markov_model_order=m)
  got = _call(rule, stream_a, stream_b, markov_model_order=order)
  assert isinstance(got, bytes)
  assert got == want, f"{expected.shape} {expected.dtype} rule={rule} order={order}"
  out = crackle_amd.header(got)
  # (the order is in the bytes compared above: compress itself writes order 0 into the stream of a volume without cracks)
  assert out.label_format == 0 and out.format_version == 1 and out.fortran_order == head.fortran_order
  assert out.data_width == expected.dtype.itemsize and not out.signed
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


def _combine_and_check(a, b, checker, rule, order=None, kw_a=None, kw_b=None):
  return _check(_compress(a, checker, **(kw_a or {})), _compress(b, checker, **(kw_b or {})), combine_numpy.combine(a, b, rule), checker, rule, order=order)


def _all_rules(a, b, checker, **kw):
  return [_combine_and_check(a, b, checker, rule, **kw) for rule in RULES]


# ---- word and row edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", volumes.EDGE_VARIANTS)
@pytest.mark.parametrize("sx", volumes.EDGE_SX)
def test_word_and_row_edges(sx, variant, checker):
  """Every sy, sz of 1 .. 4 under the three rules, byte for byte; all of the checks on the largest."""
  for sy in volumes.EDGE_SYZ:
    for sz in volumes.EDGE_SYZ:
      a, b = volumes.edges((sx, sy, sz), variant)
      sa, sb = _compress(a, checker), _compress(b, checker)
      for rule in RULES:
        want = checker.compress(combine_numpy.combine(a, b, rule), fortran_order=True)
        assert _call(rule, sa, sb) == want, f"{a.shape} {variant} rule={rule}"
  for shape in ((sx, 4, 4), (sx, 3, 3)):
    _all_rules(*volumes.edges(shape, variant), checker)


# ---- hand-built rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,da,db,row_a,row_b,over,keep,drop", volumes.HAND, ids=[c[0] for c in volumes.HAND])
def test_hand_built_rows(name, da, db, row_a, row_b, over, keep, drop, checker):
  for x0 in volumes.HAND_PLACES:
    a, b = volumes.hand(da, db, row_a, row_b, x0)
    for rule, want in zip(RULES, (over, keep, drop)):
      got = _combine_and_check(a, b, checker, rule)
      assert crackle_amd.decompress(got)[x0:, 1, 0].tolist() == list(want)      # (the literal answer)


# ---- data widths -------------------------------------------------------------------------------------------------------
def test_narrow_under_wide_and_the_reverse(checker):
  a, b = volumes.narrow_and_wide()
  over, keep, drop = _all_rules(a, b, checker)
  assert crackle_amd.header(over).data_width == 8 and int(crackle_amd.decompress(over).max()) == volumes.TOP
  assert crackle_amd.header(keep).data_width == crackle_amd.header(drop).data_width == 1
  over, keep, drop = _all_rules(b, a, checker)
  assert [crackle_amd.header(s).data_width for s in (over, keep, drop)] == [8, 8, 8]
  assert int(crackle_amd.decompress(keep).max()) == volumes.TOP


@pytest.mark.parametrize("db", [np.uint8, np.uint16, np.uint32, np.uint64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("da", [np.uint8, np.uint16, np.uint32, np.uint64], ids=lambda d: np.dtype(d).name)
def test_every_unsigned_width_pair(da, db, checker):
  a, b = volumes.for_dtypes(da, db)
  over, keep, drop = _all_rules(a, b, checker, kw_a=dict(markov_model_order=2))
  assert crackle_amd.header(over).data_width == max(np.dtype(da).itemsize, np.dtype(db).itemsize)
  assert crackle_amd.header(keep).data_width == crackle_amd.header(drop).data_width == np.dtype(da).itemsize


# ---- the crack format --------------------------------------------------------------------------------------------------
def _format_bit(stream):
  return crackle_amd.header(stream).crack_format == 1


def test_streams_of_different_crack_formats(checker):
  a, b = volumes.formats_differ()
  sa, sb = _compress(a, checker), _compress(b, checker)
  assert _format_bit(sa) == permissible(a) == True and _format_bit(sb) == permissible(b) == False
  for first, second, s1, s2 in ((a, b, sa, sb), (b, a, sb, sa)):
    for rule in RULES:
      expected = combine_numpy.combine(first, second, rule)
      assert _format_bit(_check(s1, s2, expected, checker, rule)) == permissible(expected)


def test_the_crack_format_follows_the_combined_volume(checker):
  a, b = volumes.format_flips()
  sa, sb = _compress(a, checker), _compress(b, checker)
  assert _format_bit(sa) == permissible(a) == True and _format_bit(sb) == permissible(b) == True
  seen = {}
  for rule in RULES:
    expected = combine_numpy.combine(a, b, rule)
    seen[rule] = _format_bit(_check(sa, sb, expected, checker, rule))
    assert seen[rule] == permissible(expected)
  assert seen == dict(overlay=True, keep=True, drop=False)      # another format than either input's


# ---- label counts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("n", volumes.COUNTS)
def test_label_counts_around_a_byte_of_index(n, rule, checker):
  a, b = volumes.survivors(n, rule)
  sa = _compress(a, checker)
  assert crackle_amd.num_labels(sa) == 320
  got = _combine_and_check(a, b, checker, rule)
  assert crackle_amd.num_labels(got) == n
  left = crackle_amd.labels(got).tolist()
  assert 320 not in left      # A's largest label is among those that vanished
  if rule != "overlay":
    assert crackle_amd.header(got).stored_data_width == (1 if n <= 256 else 2) and crackle_amd.header(got).data_width == 2


# ---- generated ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=range(len(volumes.GENERATED)), ids=["x".join(map(str, g[0])) + g[1] for g in volumes.GENERATED])
def generated(request):
  a, b = volumes.generated(request.param)
  a.setflags(write=False)
  b.setflags(write=False)
  return a, b


@pytest.mark.parametrize("kw_b", ENCODINGS, ids=["b-" + i for i in ENCODING_IDS])
@pytest.mark.parametrize("kw_a", ENCODINGS, ids=["a-" + i for i in ENCODING_IDS])
def test_generated(generated, kw_a, kw_b, checker):
  a, b = generated
  sa = _compress(a, checker, **kw_a)
  assert crackle_amd.header(sa).label_format == (2 if kw_a.get("allow_pins") else 0) and crackle_amd.header(sa).fortran_order == bool(a.flags.f_contiguous)
  for got in _all_rules(a, b, checker, kw_a=kw_a, kw_b=kw_b):
    assert crackle_amd.header(got).markov_model_order == kw_a.get("markov_model_order", 0)      # the first stream's


@pytest.mark.parametrize("order", [0, 3])
def test_explicit_markov_order(generated, order, checker):
  a, b = generated
  for got in _all_rules(a, b, checker, order=order, kw_a=dict(markov_model_order=5), kw_b=dict(markov_model_order=2)):
    assert crackle_amd.header(got).markov_model_order == order


def test_mixed_memory_orders(checker):
  a, b = volumes.generated(0)
  c = np.ascontiguousarray(b)
  assert a.flags.f_contiguous and c.flags.c_contiguous and not c.flags.f_contiguous
  for got in _all_rules(a, c, checker):
    assert crackle_amd.header(got).fortran_order
  for got in _all_rules(c, a, checker):
    assert not crackle_amd.header(got).fortran_order


def test_many_workgroups_of_words(checker):
  _all_rules(*volumes.many_words(), checker)


@pytest.mark.parametrize("shape", [(37, 1, 1), (1, 6, 5), (1, 1, 1), (2, 2, 2), (64, 2, 2), (65, 2, 1)], ids=lambda s: "x".join(map(str, s)))
def test_small_shapes(shape, checker):
  a, b = (v[:shape[0], :shape[1], :shape[2]].copy(order="F") for v in volumes.generated(0))
  _all_rules(a, b, checker)


# ---- identities --------------------------------------------------------------------------------------------------------
def test_identities(generated, checker):
  a, _ = generated
  sa = _compress(a, checker, markov_model_order=3)
  same = crackle_amd.recompress(sa)
  assert same == _compress(a, checker, markov_model_order=3)
  assert overlay(sa, sa) == same
  assert mask_by(sa, sa) == same
  zero_stream = _compress(np.zeros_like(a), checker, markov_model_order=3)
  assert mask_by(sa, sa, invert=True) == zero_stream
  assert crackle_amd.labels(zero_stream).tolist() == [0]
  # zeros of a wider dtype: a's labels at the wider width
  zeros64 = _compress(np.zeros(a.shape, np.uint64, order="F" if a.flags.f_contiguous else "C"), checker)
  wide = overlay(sa, zeros64)
  assert wide == _compress(a.astype(np.uint64, order="K"), checker, markov_model_order=3)
  assert wide == crackle_amd.recompress(_compress(a.astype(np.uint64, order="K"), checker, markov_model_order=3))
  assert mask_by(sa, zeros64) == zero_stream and mask_by(sa, zeros64, invert=True) == same
  # CrackleArray: the same bytes, a new array, the other stream as an array or as bytes
  arr = crackle_amd.CrackleArray(sa)
  for other in (crackle_amd.CrackleArray(zeros64), zeros64):
    out = arr.overlay(other)
    assert type(out) is crackle_amd.CrackleArray and out is not arr and out.binary == wide
    assert arr.mask_by(other, invert=True).binary == same and arr.mask_by(other).binary == zero_stream


# ---- an independent check through the consumers -----------------------------------------------------------------------
def test_voxel_counts_follow_the_overlap_table(generated, checker):
  a, b = generated
  sa, sb = _compress(a, checker), _compress(b, checker, allow_pins=True)
  table = crackle_amd.overlaps(sa, sb)
  assert sum(table.values()) == a.size
  for rule in RULES:
    got = _call(rule, sa, sb)
    assert crackle_amd.voxel_counts(got) == combine_numpy.predicted_counts(table, rule), rule


# ---- both label paths of the encoder, and the profile line -------------------------------------------------------------
FIELDS = ["tables", "merge_planes", "graph", "cracks", "labels", "assembly", "k_combine_device", "pieces"]


def _profiled(capfd, monkeypatch, rule, sa, sb):
  monkeypatch.setenv("CKL_PROFILE", "1")
  capfd.readouterr()
  got = _call(rule, sa, sb)
  monkeypatch.delenv("CKL_PROFILE", raising=False)
  err = capfd.readouterr().err.splitlines()
  mine = [l for l in err if l.startswith("[ckl combine host ms]")]
  assert len(mine) == 1, err
  fields = dict(w.split("=") for w in mine[0].split()[4:])
  assert list(fields) == FIELDS, mine[0]
  assert float(fields["merge_planes"]) > 0 and float(fields["k_combine_device"]) > 0
  enc = [l for l in err if l.startswith("[ckl encode host ms]")]
  return got, sorted(w.split("=")[0] for w in enc[-1].split() if w.startswith("f:")), int(fields["pieces"])


def test_strip_path(checker, monkeypatch, capfd):
  a, b = volumes.strip_path()
  sa, sb = _compress(a, checker), _compress(b, checker)
  monkeypatch.delenv("CKL_ENC_LABEL_RUNS", raising=False)
  for rule in RULES:
    expected = combine_numpy.combine(a, b, rule)
    got = _check(sa, sb, expected, checker, rule)
    again, marks, pieces = _profiled(capfd, monkeypatch, rule, sa, sb)
    assert again == got and "f:enqueue_strips" in marks and "f:wait_strips" in marks, marks
    assert pieces == combine_numpy.x_runs(expected)
    if rule == "overlay":
      # the same pair with the run pipeline forced
      monkeypatch.setenv("CKL_ENC_LABEL_RUNS", "1")
      again, marks, pieces = _profiled(capfd, monkeypatch, rule, sa, sb)
      monkeypatch.delenv("CKL_ENC_LABEL_RUNS")
      assert again == got and "f:enqueue_runs" in marks and "f:wait_runs" in marks, marks
      assert pieces == combine_numpy.x_runs(expected)


def test_run_pipeline(checker, monkeypatch, capfd):
  a, b = volumes.run_pipeline()
  sa, sb = _compress(a, checker), _compress(b, checker)
  monkeypatch.delenv("CKL_ENC_LABEL_RUNS", raising=False)
  for rule in RULES:
    expected = combine_numpy.combine(a, b, rule)
    got = _check(sa, sb, expected, checker, rule)
    again, marks, pieces = _profiled(capfd, monkeypatch, rule, sa, sb)
    assert again == got and "f:enqueue_runs" in marks and "f:wait_runs" in marks, marks
    assert pieces == combine_numpy.x_runs(expected)


@pytest.mark.parametrize("rule", RULES)
def test_profile_line(rule, generated, checker, monkeypatch, capfd):
  a, b = generated
  expected = combine_numpy.combine(a, b, rule)
  got, _, pieces = _profiled(capfd, monkeypatch, rule, _compress(a, checker), _compress(b, checker))
  assert got == checker.compress(expected, fortran_order=bool(a.flags.f_contiguous))
  assert pieces == combine_numpy.x_runs(expected) > expected.shape[1] * expected.shape[2]


# ---- false boundaries --------------------------------------------------------------------------------------------------
def _with_and_without_false_boundaries(dirty, volume, checker):
  """dirty: a stream of `volume` with false boundaries.  As A and as B it gives what its recompressed form gives."""
  clean = crackle_amd.recompress(dirty)
  assert len(clean) < len(dirty)
  other = volumes.second(volume.shape, offset=100)
  so = _compress(other, checker)
  for rule in RULES:
    got = _check(dirty, so, combine_numpy.combine(volume, other, rule), checker, rule)
    assert _call(rule, clean, so) == got
    got = _check(so, dirty, combine_numpy.combine(other, volume, rule), checker, rule)
    assert _call(rule, so, clean) == got


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


# ---- every kind of stream ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kinds(checker):
  vol = stream_kinds.volume_a()
  return {k.name: k for k in stream_kinds.kinds_host(vol, checker) + stream_kinds.kinds_device(vol, checker)}


@pytest.mark.parametrize("name", stream_kinds.HOST_KINDS + stream_kinds.DEVICE_KINDS)
def test_every_stream_kind(name, kinds, checker):
  kind = kinds[name]
  other = _compress(kind.other, checker)
  for rule in RULES:      # (kind.other holds no 0: the direction in which the rules have work to do is the second)
    _check(kind.stream, other, combine_numpy.combine(kind.expected, kind.other, rule), checker, rule)
    _check(other, kind.stream, combine_numpy.combine(kind.other, kind.expected, rule), checker, rule)


def test_version_0_stream(checker):
  with np.load(os.path.join(HERE, "golden", "v0.npz")) as z:
    b0 = z[sorted(k for k in z.files if "." not in k)[0]].tobytes()
  head = crackle_amd.header(b0)
  assert head.format_version == 0 and not head.signed
  arr = checker.decompress(b0).reshape((head.sx, head.sy, head.sz), order="F" if head.fortran_order else "C")
  other = combine_numpy.like(arr, np.where(arr % 3 == 0, 0, arr // 2 + 1).astype(arr.dtype))
  assert (other == 0).any() and (other != 0).any()
  so = _compress(other, checker)
  for rule in RULES:
    _check(b0, so, combine_numpy.combine(arr, other, rule), checker, rule)
    _check(so, b0, combine_numpy.combine(other, arr, rule), checker, rule)
  assert overlay(b0, b0) == crackle_amd.recompress(b0)


# ---- repeatability and damage ------------------------------------------------------------------------------------------
def test_repeatable(checker):
  a, b = volumes.many_words()
  sa, sb = _compress(a, checker, markov_model_order=4), _compress(b, checker)
  for rule in RULES:
    outs = [_call(rule, sa, sb) for _ in range(3)]
    assert outs[0] == outs[1] == outs[2] == checker.compress(combine_numpy.combine(a, b, rule), markov_model_order=4)


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


def test_errors_on_the_device_side(checker):
  a = erode_volumes.voronoi((48, 40, 5), dtype=np.uint16, cell=(8, 8, 2))
  b = volumes.second((48, 40, 5), dtype=np.uint16, offset=100)
  sa, sb = _compress(a, checker), _compress(b, checker)
  bad_a, error_a = _damaged(sa, 2)
  bad_b, error_b = _damaged(sb, 3)
  assert str(error_a) != str(error_b)
  for rule in RULES:
    for first, second, error in ((bad_a, sb, error_a), (sa, bad_b, error_b), (bad_a, bad_b, error_a)):      # both damaged: the first stream's error wins
      with pytest.raises(type(error), match=re.escape(str(error))):
        _call(rule, first, second)
      assert _call(rule, sa, sb) == checker.compress(combine_numpy.combine(a, b, rule))      # the session pool is none the worse for it
