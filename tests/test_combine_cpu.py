"""overlay and mask_by without a GPU: the restatement (tests/combine_numpy.py) pinned by a literal triple loop and by the
literal answers of the hand-built rows; what the pairs of tests/combine_volumes.py hold (none of them is vacuous); the
public surface, the refusals decided on the host (through Python and through the C entry), and streams without voxels."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import crackle_amd
import combine_numpy
import combine_volumes as volumes
from crackle_amd import _lib, operations
from crackle_amd import overlay, mask_by      # (the feature under test: without it nothing here runs)
from recompress_volumes import as_signed, permissible
from util import golden

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RULES = combine_numpy.RULES
RULE_CODES = {"overlay": 0, "keep": 1, "drop": 2}


def _restate(a, b, rule):
  out = combine_numpy.combine(a, b, rule)
  assert out.shape == a.shape and out.dtype == combine_numpy.out_dtype(a.dtype, b.dtype, rule)
  if a.flags.f_contiguous != a.flags.c_contiguous and out.flags.f_contiguous != out.flags.c_contiguous:
    assert out.flags.f_contiguous == a.flags.f_contiguous
  return out


# ---- the restatement ---------------------------------------------------------------------------------------------------
def _triple_loop(a, b, rule):
  width = max(a.dtype.itemsize, b.dtype.itemsize) if rule == "overlay" else a.dtype.itemsize
  out = np.zeros(a.shape, {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[width], order="F")
  for x in range(a.shape[0]):
    for y in range(a.shape[1]):
      for z in range(a.shape[2]):
        va, vb = int(a[x, y, z]), int(b[x, y, z])
        if rule == "overlay":
          out[x, y, z] = vb if vb != 0 else va
        elif rule == "keep":
          out[x, y, z] = va if vb != 0 else 0
        else:
          out[x, y, z] = 0 if vb != 0 else va
  return out


@pytest.mark.parametrize("rule", RULES)
def test_restatement_is_the_literal_triple_loop(rule):
  rng = np.random.default_rng(97 + RULE_CODES[rule])
  for shape in ((9, 7, 5), (1, 6, 5), (12, 1, 1), (1, 1, 1)):
    for da, db in ((np.uint8, np.uint8), (np.uint16, np.uint8), (np.uint8, np.uint32), (np.uint64, np.uint16), (np.uint8, np.uint64)):
      a = np.asfortranarray(rng.integers(0, 5, shape).astype(da))
      b = np.asfortranarray(rng.choice(np.array([0, 0, 3, np.iinfo(db).max], db), shape))
      assert np.array_equal(_restate(a, b, rule), _triple_loop(a, b, rule)), (shape, da, db)
      c_order = np.ascontiguousarray(a)
      out = _restate(c_order, np.ascontiguousarray(b), rule)
      assert np.array_equal(out, _triple_loop(a, b, rule)) and out.flags.c_contiguous
  assert np.array_equal(combine_numpy.overlay(a, b), _restate(a, b, "overlay"))
  assert np.array_equal(combine_numpy.mask_by(a, b), _restate(a, b, "keep")) and np.array_equal(combine_numpy.mask_by(a, b, invert=True), _restate(a, b, "drop"))


def test_restated_dtypes():
  for rule in RULES:
    for wa in (1, 2, 4, 8):
      for wb in (1, 2, 4, 8):
        want = max(wa, wb) if rule == "overlay" else wa
        assert combine_numpy.out_dtype("u%d" % wa, "u%d" % wb, rule) == np.dtype("u%d" % want)


def test_restated_runs_and_predicted_counts():
  row = np.array([1, 1, 2, 2, 2, 1, 0], np.uint8).reshape((7, 1, 1), order="F")
  assert combine_numpy.x_runs(row) == 4
  assert combine_numpy.x_runs(np.repeat(np.repeat(row, 3, axis=1), 2, axis=2)) == 24
  assert combine_numpy.x_runs(np.zeros((5, 4, 3), np.uint8)) == 12
  table = {(1, 0): 4, (1, 9): 2, (0, 9): 3, (0, 0): 5, (2, 8): 1}
  assert combine_numpy.predicted_counts(table, "overlay") == {1: 4, 9: 5, 0: 5, 8: 1}
  assert combine_numpy.predicted_counts(table, "keep") == {0: 12, 1: 2, 2: 1}
  assert combine_numpy.predicted_counts(table, "drop") == {1: 4, 0: 11}


@pytest.mark.parametrize("name,da,db,row_a,row_b,over,keep,drop", volumes.HAND, ids=[c[0] for c in volumes.HAND])
def test_restatement_hand_built_rows(name, da, db, row_a, row_b, over, keep, drop):
  assert len({len(r) for r in (row_a, row_b, over, keep, drop)}) == 1
  for x0 in volumes.HAND_PLACES:
    a, b = volumes.hand(da, db, row_a, row_b, x0)
    assert a.shape == b.shape == (x0 + len(row_a), 3, 2) and a.dtype == da and b.dtype == db
    assert a[x0:, 1, 0].tolist() == list(row_a) and b[x0:, 1, 0].tolist() == list(row_b)
    for rule, want in zip(RULES, (over, keep, drop)):
      out = _restate(a, b, rule)
      assert out[x0:, 1, 0].tolist() == list(want), (name, rule)
      background = volumes.HAND_BACKGROUND[0] if rule != "keep" else 0
      assert (out[:, 0, :] == background).all() and (out[:, :, 1] == background).all()


# ---- what the GPU tests rely on ----------------------------------------------------------------------------------------
def _not_vacuous(a, b):
  """Every rule changes something, the two masks keep something, and B has zeros and labels."""
  assert (b == 0).any() and (b != 0).any()
  for rule in RULES:
    out = _restate(a, b, rule)
    assert not np.array_equal(out, a), rule
    assert out.any(), rule
  assert not np.array_equal(_restate(a, b, "overlay"), b.astype(_restate(a, b, "overlay").dtype))


@pytest.mark.parametrize("i", range(len(volumes.GENERATED)), ids=["x".join(map(str, g[0])) + g[1] for g in volumes.GENERATED])
def test_generated_pairs_are_not_vacuous(i):
  shape, order = volumes.GENERATED[i]
  a, b = volumes.generated(i)
  for v in (a, b):
    assert v.shape == shape and v.flags.c_contiguous == (order == "C") and v.flags.f_contiguous == (order == "F")
  _not_vacuous(a, b)
  assert 0.35 < np.count_nonzero(b) / b.size < 0.65      # about half of B is background
  out = _restate(a, b, "overlay")
  left = np.unique(out)
  assert int(a.max()) < 40 and int(b[b != 0].min()) > 100
  assert (left < 40).sum() > 20 and (left > 100).sum() > 10      # labels of both inputs
  assert combine_numpy.x_runs(out) > combine_numpy.x_runs(b) > shape[1] * shape[2]


def _changes(row):
  return tuple((np.flatnonzero(row[1:] != row[:-1]) + 1).tolist())


@pytest.mark.parametrize("variant", volumes.EDGE_VARIANTS)
def test_edge_pairs_hold_the_breaks_they_claim(variant):
  for sx in volumes.EDGE_SX:
    for shape in ((sx, 4, 3), (sx, 1, 1)):
      a, b = volumes.edges(shape, variant)
      assert a.shape == b.shape == shape and a.dtype == b.dtype == np.uint8
      for y in range(shape[1]):
        for z in range(shape[2]):
          ra, rb = _changes(a[:, y, z]), _changes(b[:, y, z])
          if variant == "one-pixel-labels":
            assert ra == rb == tuple(range(1, sx))
            continue
          want_a, want_b = volumes.breaks_of(variant, sx)
          assert ra == (() if variant == "a-uniform" else want_a), (variant, sx, y, z)
          assert rb == (() if variant in ("b-zero", "b-full") else want_b), (variant, sx, y, z)
      if shape[1] > 1 and variant != "a-uniform":
        assert not np.array_equal(a[:, 0, 0], a[:, 1, 0]) and not np.array_equal(a[:, :, 0], a[:, :, 1])      # the rows and slices differ
  assert volumes.breaks_of("same-column", 65)[0] == volumes.breaks_of("same-column", 65)[1] != ()
  a65, b65 = volumes.breaks_of("adjacent-columns", 65)
  assert tuple(c + 1 for c in a65) == b65 and {31, 63} <= set(a65)
  assert volumes.breaks_of("bit31-bit0", 65) == ((31,), (32,)) and volumes.breaks_of("bit31-bit0", 32) == ((31,), ())
  assert all(c < 32 for side in volumes.breaks_of("carried", 65) for c in side)      # nothing in the second and third words
  a, b = volumes.edges((65, 4, 3), "b-zero")
  assert not b.any() and np.array_equal(_restate(a, b, "overlay"), a) and not _restate(a, b, "keep").any()
  a, b = volumes.edges((65, 4, 3), "b-full")
  assert (b == 9).all() and (_restate(a, b, "overlay") == 9).all() and not _restate(a, b, "drop").any()
  a, b = volumes.edges((65, 4, 3), "a-uniform")
  assert (a == 4).all()
  for variant in ("same-column", "adjacent-columns", "bit31-bit0", "carried", "a-uniform", "one-pixel-labels"):
    _not_vacuous(*volumes.edges((65, 4, 3), variant))


def test_width_pairs_are_what_they_say():
  a, b = volumes.narrow_and_wide()
  assert a.dtype == np.uint8 and b.dtype == np.uint64 and a.shape == b.shape
  labels = np.unique(b).tolist()
  assert labels[0] == 0 and labels[-1] == volumes.TOP == 2**64 - 1 and any((1 << 32) < v < volumes.TOP for v in labels)
  _not_vacuous(a, b)
  _not_vacuous(b, a)
  assert _restate(a, b, "overlay").dtype == _restate(b, a, "overlay").dtype == np.uint64
  assert int(_restate(a, b, "overlay").max()) == volumes.TOP and _restate(a, b, "keep").dtype == np.uint8 and _restate(b, a, "keep").dtype == np.uint64
  for da in (np.uint8, np.uint16, np.uint32, np.uint64):
    for db in (np.uint8, np.uint16, np.uint32, np.uint64):
      a, b = volumes.for_dtypes(da, db)
      assert a.dtype == da and b.dtype == db
      _not_vacuous(a, b)
      if da == np.uint64:
        assert int(a.max()) > 1 << 40
      if db == np.uint64:
        assert int(b.max()) > 1 << 40


def test_format_pairs_are_what_they_say():
  a, b = volumes.formats_differ()
  assert permissible(a) and not permissible(b)
  _not_vacuous(a, b)
  a, b = volumes.format_flips()
  assert permissible(a) and permissible(b)
  assert permissible(_restate(a, b, "overlay")) and permissible(_restate(a, b, "keep"))
  assert not permissible(_restate(a, b, "drop"))      # another format than either input
  _not_vacuous(a, b)


@pytest.mark.parametrize("n", volumes.COUNTS)
def test_label_count_pairs_are_what_they_say(n):
  for rule in RULES:
    a, b = volumes.survivors(n, rule)
    assert a.shape == b.shape == volumes.COUNT_SHAPE and a.dtype == np.uint16
    assert np.unique(a).size == 320 and int(a.max()) == 320
    out = _restate(a, b, rule)
    left = np.unique(out)
    assert left.size == n, (rule, left.size)
    assert 320 not in left.tolist() and np.setdiff1d(np.unique(a), left).size >= 320 - n      # labels of A vanish, its largest among them
    if rule == "overlay":
      assert set(left.tolist()) & set(np.unique(a).tolist()) and set(left.tolist()) & set(np.unique(b).tolist())      # drawn from both inputs
      assert int(left.max()) >= 5000
    else:
      assert int(left.max()) == n - 1      # 256 labels: the largest survivor fits one byte, 257: it does not
      assert int(b.max()) == 7 and b.dtype == np.uint8


def test_other_pairs_are_what_they_say():
  a, b = volumes.many_words()
  assert a.shape == volumes.MANY_WORDS and -(-a.shape[0] // 32) * a.shape[1] > 256
  _not_vacuous(a, b)
  a, b = volumes.strip_path()
  assert a.shape == b.shape == (320, 288, 5)
  _not_vacuous(a, b)
  a, b = volumes.run_pipeline()
  assert a.shape == b.shape == (32800, 3, 2) and a.dtype == b.dtype == np.uint8
  _not_vacuous(a, b)


# ---- the surface -------------------------------------------------------------------------------------------------------
NOT_DONE = ("Not done: where(cond, a, b) over three streams, a joint (product) segmentation with fresh ids, a fill value other than 0, z-ranges, "
            "a sharded version, a place in the thread-job and stream-kind matrices of the existing test files.")


def test_surface():
  assert crackle_amd.overlay is operations.overlay is overlay and crackle_amd.mask_by is operations.mask_by is mask_by
  assert "overlay" in crackle_amd.__all__ and "mask_by" in crackle_amd.__all__
  sig = inspect.signature(crackle_amd.overlay)
  assert list(sig.parameters) == ["binary", "other", "markov_model_order", "device"] and [p.default for p in sig.parameters.values()][2:] == [None, 0]
  sig = inspect.signature(crackle_amd.mask_by)
  assert list(sig.parameters) == ["binary", "other", "invert", "markov_model_order", "device"] and [p.default for p in sig.parameters.values()][2:] == [False, None, 0]
  sig = inspect.signature(crackle_amd.CrackleArray.overlay)
  assert list(sig.parameters) == ["self", "other"]
  sig = inspect.signature(crackle_amd.CrackleArray.mask_by)
  assert list(sig.parameters) == ["self", "other", "invert"] and sig.parameters["invert"].default is False
  text = open(os.path.join(ROOT, "include", "crackle_amd.h")).read()
  assert re.search(r"\bint\s+ckl_combine\s*\(\s*const uint8_t\*\s*buf_a,\s*uint64_t n_a,\s*const uint8_t\*\s*buf_b,\s*uint64_t n_b,\s*int rule,\s*int flags[^,]*,\s*"
                   r"int markov_model_order[^,]*,\s*int device,\s*uint8_t\*\*\s*out,\s*uint64_t\*\s*out_len\s*\)", text)
  for name, value in (("CKL_COMBINE_OVERLAY", 0), ("CKL_COMBINE_KEEP_WHERE", 1), ("CKL_COMBINE_DROP_WHERE", 2)):
    assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text) and getattr(_lib, name) == value
  assert _lib.EXPORTS["ckl_combine"] == (C.c_int, [
    C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)])
  assert hasattr(C.CDLL(_lib.LIB_PATH), "ckl_combine")
  assert _lib.lib().ckl_abi_version() == 1      # an entry was added, none changed
  for fn in (operations.overlay, operations.mask_by):
    doc = " ".join(fn.__doc__.split())
    assert doc.endswith(NOT_DONE), fn.__name__
    for words in ("byte for byte", "FLAT labels, format version 1", "the crack format the combined volume itself selects", "Equality is by label"):
      assert words in doc, (fn.__name__, words)
  doc = " ".join(operations.overlay.__doc__.split())
  for words in ("V = B where B != 0, else A", "the larger of the two streams' data widths", "Label 0 of `other` is the only special value", "binary's first"):
    assert words in doc, words
  doc = " ".join(operations.mask_by.__doc__.split())
  for words in ("V = A where (B != 0) != invert, else 0", "other's labels never appear"):
    assert words in doc, words


def test_array_methods_pass_the_other_stream_on(monkeypatch):
  calls = []
  monkeypatch.setattr(operations, "overlay", lambda binary, other, **kw: calls.append(("overlay", binary, other, kw)) or binary)
  monkeypatch.setattr(operations, "mask_by", lambda binary, other, **kw: calls.append(("mask_by", binary, other, kw)) or binary)
  a, b = golden()["c0_voronoi_u8"], golden()["c0_voronoi_u8"] + b"\0"      # (told apart by their length; the fakes return a itself)
  arr, other = crackle_amd.CrackleArray(a, device=0), crackle_amd.CrackleArray(b, device=0)
  for given in (other, b):
    out = arr.overlay(given)
    assert type(out) is crackle_amd.CrackleArray and out.binary == a and out is not arr
    out = arr.mask_by(given, invert=True)
    assert type(out) is crackle_amd.CrackleArray and out.binary == a and out is not arr
    assert arr.mask_by(given).binary == a
  assert calls == [("overlay", a, b, dict(device=0)), ("mask_by", a, b, dict(invert=True, device=0)), ("mask_by", a, b, dict(invert=False, device=0))] * 2


def _calls(a, b, **kw):
  """Every public way to the three rules."""
  return [lambda: crackle_amd.overlay(a, b, **kw), lambda: crackle_amd.mask_by(a, b, **kw), lambda: crackle_amd.mask_by(a, b, invert=True, **kw)]


def test_refusals_need_no_device(checker):
  binary = golden()["c0_voronoi_u8"]
  head = crackle_amd.header(binary)
  shape = (head.sx, head.sy, head.sz)
  out, n = C.c_void_p(), C.c_uint64()
  L = _lib.lib()

  def entry(a, b, rule=0, flags=0, order=-1):
    rc = L.ckl_combine(a, len(a), b, len(b), rule, flags, order, 0, C.byref(out), C.byref(n))
    assert out.value is None and n.value == 0
    return rc, L.ckl_last_error().decode()

  # shapes differ: overlaps' wording with both shapes
  for other_shape in ((shape[0] + 1, shape[1], shape[2]), (shape[0], shape[1] - 1, shape[2]), (shape[0], shape[1], shape[2] + 2)):
    other = checker.compress(np.zeros(other_shape, np.uint8, order="F"))
    told = "the volumes differ in shape: %d x %d x %d and %d x %d x %d" % (shape + other_shape)
    for call, what in zip(_calls(binary, other), ("overlay", "mask_by", "mask_by")):
      with pytest.raises(ValueError, match=re.escape(what + ": " + told)):
        call()
    with pytest.raises(ValueError, match=re.escape("overlay: the volumes differ in shape: %d x %d x %d and %d x %d x %d" % (other_shape + shape))):
      crackle_amd.CrackleArray(other).overlay(binary)
    with pytest.raises(ValueError, match=re.escape(told)):
      crackle_amd.CrackleArray(binary).mask_by(crackle_amd.CrackleArray(other))
    for rule, what in ((0, "overlay"), (1, "mask_by"), (2, "mask_by")):
      rc, said = entry(binary, other, rule)
      assert rc == _lib.CKL_ERR_ARG and (what + ": " + told) in said
  # signed streams, on either side
  signed = as_signed(binary)
  assert crackle_amd.header(signed).signed
  for a, b in ((signed, binary), (binary, signed), (signed, signed)):
    for call in _calls(a, b):
      with pytest.raises(TypeError, match="Signed integer data types are not currently supported."):
        call()
    with pytest.raises(TypeError):
      crackle_amd.CrackleArray(a).overlay(b)
    for rule in (0, 1, 2):
      rc, said = entry(a, b, rule)
      assert rc == _lib.CKL_ERR_ARG and "Signed integer data types are not currently supported." in said
  # the order
  for call, what in zip(_calls(binary, binary, markov_model_order=-1), ("overlay", "mask_by", "mask_by")):
    with pytest.raises(ValueError, match=what + ": markov_model_order must not be negative"):
      call()
  with pytest.raises(ValueError) as seen:
    crackle_amd.recompress(binary, markov_model_order=16)
  for call in _calls(binary, binary, markov_model_order=16):
    with pytest.raises(ValueError, match=re.escape(str(seen.value))):      # the road's own error
      call()
  rc, said = entry(binary, binary, 0, 0, 16)
  assert rc == _lib.CKL_ERR_ARG and said == str(seen.value)
  # the C entry alone: rule, flags, null pointers
  for rule in (-1, 3, 17):
    rc, said = entry(binary, binary, rule)
    assert rc == _lib.CKL_ERR_ARG and "unknown rule" in said
  for flags in (1, 2, -1):
    rc, said = entry(binary, binary, 0, flags)
    assert rc == _lib.CKL_ERR_ARG and "flags must be 0" in said
  k = len(binary)
  assert L.ckl_combine(None, 0, binary, k, 0, 0, -1, 0, C.byref(out), C.byref(n)) == _lib.CKL_ERR_ARG
  assert L.ckl_combine(binary, k, None, 0, 0, 0, -1, 0, C.byref(out), C.byref(n)) == _lib.CKL_ERR_ARG
  assert L.ckl_combine(binary, k, binary, k, 0, 0, -1, 0, None, C.byref(n)) == _lib.CKL_ERR_ARG
  assert L.ckl_combine(binary, k, binary, k, 0, 0, -1, 0, C.byref(out), None) == _lib.CKL_ERR_ARG
  assert L.ckl_combine(binary[:10], 10, binary, k, 0, 0, -1, 0, C.byref(out), C.byref(n)) != _lib.CKL_OK
  assert L.ckl_combine(binary, k, binary[:10], 10, 0, 0, -1, 0, C.byref(out), C.byref(n)) != _lib.CKL_OK
  assert out.value is None and n.value == 0


@pytest.mark.parametrize("shape", [(0, 0, 0), (5, 0, 3), (4, 4, 0)], ids=lambda s: "x".join(map(str, s)))
def test_streams_without_voxels(checker, shape):
  a = checker.compress(np.zeros(shape, np.uint16, order="F"), markov_model_order=3)
  wide = checker.compress(np.zeros(shape, np.uint64, order="F"))
  narrow = checker.compress(np.zeros(shape, np.uint8, order="C"), fortran_order=False)
  empty16 = np.zeros(shape, np.uint16, order="F")
  want = checker.compress(empty16, markov_model_order=3)
  for call in _calls(a, narrow):
    assert call() == want
  for call in _calls(a, narrow, markov_model_order=0):
    assert call() == checker.compress(empty16)
  # overlay takes the wider of the two widths, the masks keep a's; the order flag and the order are a's
  assert crackle_amd.overlay(a, wide) == checker.compress(np.zeros(shape, np.uint64, order="F"), markov_model_order=3)
  assert crackle_amd.mask_by(a, wide) == crackle_amd.mask_by(a, wide, invert=True) == want
  assert crackle_amd.overlay(narrow, a) == checker.compress(np.zeros(shape, np.uint16, order="C"), fortran_order=False)
  assert crackle_amd.mask_by(narrow, a) == checker.compress(np.zeros(shape, np.uint8, order="C"), fortran_order=False)
  assert crackle_amd.CrackleArray(a).overlay(crackle_amd.CrackleArray(narrow)).binary == want
  assert crackle_amd.CrackleArray(a).mask_by(narrow, invert=True).binary == want
  head = crackle_amd.header(want)
  assert (head.sx, head.sy, head.sz) == shape
  # the C entry answers from the host alone too
  out, n = C.c_void_p(), C.c_uint64()
  L = _lib.lib()
  for rule in (0, 1, 2):
    assert L.ckl_combine(a, len(a), narrow, len(narrow), rule, 0, -1, 0, C.byref(out), C.byref(n)) == _lib.CKL_OK
    try:
      assert C.string_at(out.value, n.value) == want
    finally:
      L.ckl_free(out)
