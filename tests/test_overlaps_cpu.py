"""overlaps without a GPU: the numpy restatement (tests/overlaps_numpy.py) against tables written out by
hand, the partition invariants on every volume the GPU tests use, the properties of those volumes
that the GPU tests rely on, and what the two C entry points (ckl_decoder_overlaps, ckl_overlaps) and
crackle_amd.overlaps decide before any device work."""
import ctypes as C

import numpy as np
import pytest

import crackle_amd
from crackle_amd import _lib, operations
import overlaps_numpy as on


# ---- the restatement ---------------------------------------------------------------------------------------------
def test_hand_written_tables():
  # 2 x 2 x 1: every voxel a pair of its own but two
  a = np.array([[[1], [1]], [[2], [0]]], np.uint8)      # a[x, y, z]
  b = np.array([[[7], [7]], [[7], [0]]], np.uint16)
  assert on.overlaps_numpy(a, b) == {(0, 0): 1, (1, 7): 2, (2, 7): 1}
  # the pair is ordered, and 0 is a label on both sides
  assert on.overlaps_numpy(b, a) == {(0, 0): 1, (7, 1): 2, (7, 2): 1}

  # 3 x 1 x 2, signed against unsigned, and a z-range
  a = np.array([[[-3, 0]], [[-3, 0]], [[2, 2]]], np.int8)
  b = np.array([[[5, 5]], [[6, 5]], [[6, 5]]], np.uint32)
  assert on.overlaps_numpy(a, b) == {(0, 5): 2, (2, 5): 1, (2, 6): 1, (2**64 - 3, 5): 1, (2**64 - 3, 6): 1}
  assert on.overlaps_numpy(a, b, 1, 2) == {(0, 5): 2, (2, 5): 1}
  assert on.overlaps_numpy(a, b, 0, 1) == {(2, 6): 1, (2**64 - 3, 5): 1, (2**64 - 3, 6): 1}

  # 4 x 2 x 1: one label against four columns, and a volume against itself (diagonal)
  a = np.full((4, 2, 1), 9, np.uint64)
  b = np.arange(4, dtype=np.uint8).reshape(4, 1, 1).repeat(2, axis=1)
  assert on.overlaps_numpy(a, b) == {(9, 0): 2, (9, 1): 2, (9, 2): 2, (9, 3): 2}
  assert on.overlaps_numpy(b, b) == {(0, 0): 2, (1, 1): 2, (2, 2): 2, (3, 3): 2}


def test_partition_invariants_on_every_builder():
  for name, (a, b) in on.small_pairs().items():
    assert a.shape == b.shape, name
    on.check_partition(on.overlaps_numpy(a, b), a, b)
    sz = a.shape[2]
    if sz > 1:
      on.check_partition(on.overlaps_numpy(a, b, sz // 2, sz), a, b, sz // 2, sz)
    assert on.swapped(on.overlaps_numpy(a, b)) == on.overlaps_numpy(b, a), name


# ---- what the GPU tests rely on ----------------------------------------------------------------------------------
def test_crack_format_pair_has_both_formats(checker):
  a, b = on.crack_format_pair()
  assert crackle_amd.header(checker.compress(a)).crack_format == crackle_amd.CrackFormat.IMPERMISSIBLE
  assert crackle_amd.header(checker.compress(b)).crack_format == crackle_amd.CrackFormat.PERMISSIBLE


def test_pin_streams_have_pin_labels(checker):
  flat = crackle_amd.LabelFormat.FLAT
  a, b = on.pin_pair()
  assert crackle_amd.header(checker.compress(a, allow_pins=True)).label_format != flat
  assert 777 not in np.unique(a)      # bgcolor=777 is then a colour outside the unique list
  for shape, oa, ob in on.GEOMETRY:
    a, b = on.geometry_pair(shape, oa, ob)
    assert crackle_amd.header(checker.compress(a, allow_pins=True)).label_format != flat, shape
    assert crackle_amd.header(checker.compress(b, allow_pins=True)).label_format != flat, shape
  # (seven labels are cheapest as FLAT keys of one byte: allow_pins on the signed volumes asks, the encoder declines)
  for name, (a, _) in on.signed_pairs().items():
    assert a.min() == -3 and a.max() == 3 and crackle_amd.header(checker.compress(a, allow_pins=True)).signed, name


def test_geometry_orders_and_word_boundary(checker):
  a, b = on.geometry_pair((96, 80, 6), "C", "F")
  ha, hb = crackle_amd.header(checker.compress(a)), crackle_amd.header(checker.compress(b))
  assert not ha.fortran_order and hb.fortran_order
  # 33 pixels a row: bit 0 of the second plane word is the only valid one, and runs of both volumes cross into it
  a, b = on.geometry_pair((33, 20, 3))
  assert np.any(a[31] == a[32]) and np.any(b[31] == b[32])
  a, b = on.one_label_pair()
  assert len(np.unique(a)) == 1 and len(np.unique(b)) == 50


def test_many_pairs_overflow_both_tables():
  """The rule of overlap_first_capacity (ckl_operations.hip), repeated: 3000 labels a side give a first
  global table of 32768 entries, and the volume has more pairs than that, and far more than the LDS
  table's 1024 entries in the 2048 runs of one workgroup."""
  a, b = on.many_pairs()
  na, nb = len(np.unique(a)), len(np.unique(b))
  assert na == nb == 3000
  assert on.first_capacity(na, nb) == 32768
  want = on.overlaps_numpy(a, b)
  assert len(want) > on.first_capacity(na, nb)
  # a workgroup takes 2048 consecutive runs of a slice, which are at least 2048 pixels: the first 21 rows
  # (2016 pixels) are fewer than that and already hold more pairs than the LDS table has entries
  assert len(on.overlaps_numpy(a[:, :21, :1], b[:, :21, :1])) > on.LDS_ENTRIES
  a, b = on.many_pairs_mixed_widths()
  assert len(on.overlaps_numpy(a, b)) > 16 * on.LDS_ENTRIES
  assert len(np.unique(a)) > 0xFF and a.dtype == np.uint16 and b.dtype == np.uint32


def test_first_capacity_rule():
  assert on.first_capacity(1, 1) == 1024
  assert on.first_capacity(4096, 32768) == 262144      # the C1 pair of the timing tool: 4 * 32768 + 4096 pairs at 3/4
  assert on.first_capacity(2, 100000) == 524288        # at most every pair: 200000
  assert on.first_capacity(100000, 2) == 524288


# ---- the ABI without a device ---------------------------------------------------------------------------------------
def _call(b1, b2, z0=0, z1=-1):
  L = _lib.lib()
  pp, cp, n = C.c_void_p(), C.c_void_p(), C.c_uint64(99)
  rc = L.ckl_overlaps(b1, len(b1), b2, len(b2), z0, z1, 0, C.byref(pp), C.byref(cp), C.byref(n))
  for p in (pp, cp):
    if p.value:
      L.ckl_free(p)
  return rc, int(n.value), bool(pp.value), bool(cp.value)


def test_symbols_and_signatures():
  L = _lib.lib()
  assert L.ckl_abi_version() == 1
  ptr, u64p = C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)
  assert _lib.EXPORTS["ckl_decoder_overlaps"] == (C.c_int, [C.c_void_p, C.c_void_p, ptr, ptr, u64p])
  assert _lib.EXPORTS["ckl_overlaps"] == (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int64, C.c_int64, C.c_int, ptr, ptr, u64p])
  for name in ("ckl_decoder_overlaps", "ckl_overlaps"):
    f = getattr(L, name)
    assert f.restype is C.c_int and list(f.argtypes) == _lib.EXPORTS[name][1]
  assert crackle_amd.overlaps is operations.overlaps and "overlaps" in crackle_amd.__all__
  assert callable(crackle_amd.CrackleArray.overlaps)


def test_null_arguments(checker):
  L = _lib.lib()
  b = checker.compress(np.ones((4, 3, 5), np.uint16, order="F"))
  pp, cp, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
  good = [b, len(b), b, len(b), 0, -1, 0, C.byref(pp), C.byref(cp), C.byref(n)]
  for i in (0, 2, 7, 8, 9):
    args = list(good)
    args[i] = None
    assert L.ckl_overlaps(*args) == _lib.CKL_ERR_ARG, i
    assert "null argument" in _lib.last_error()
  for args in ((None, None, C.byref(pp), C.byref(cp), C.byref(n)),):
    assert L.ckl_decoder_overlaps(*args) == _lib.CKL_ERR_ARG
    assert "null" in _lib.last_error()
  assert not pp.value and not cp.value


def test_shape_mismatch_is_refused_from_the_headers(checker):
  a = checker.compress(np.ones((4, 3, 5), np.uint16, order="F"))
  for shape in ((5, 3, 5), (4, 2, 5), (4, 3, 6)):
    b = checker.compress(np.ones(shape, np.uint8, order="F"))
    rc, n, p, c = _call(a, b)
    assert rc == _lib.CKL_ERR_ARG and n == 0 and not p and not c
    msg = _lib.last_error()
    assert "4 x 3 x 5" in msg and "%d x %d x %d" % shape in msg
    with pytest.raises(ValueError) as e:
      crackle_amd.overlaps(a, b)
    assert "4 x 3 x 5" in str(e.value) and "%d x %d x %d" % shape in str(e.value)
    with pytest.raises(ValueError):
      crackle_amd.CrackleArray(b).overlaps(crackle_amd.CrackleArray(a))
    with pytest.raises(ValueError):
      crackle_amd.CrackleArray(b).overlaps(a)


def test_range_errors_before_device_work(checker):
  none = checker.compress(np.zeros((0, 0, 0), np.uint8, order="F"))
  rc, n, _, _ = _call(none, none)
  assert rc == _lib.CKL_ERR_RUNTIME and _lib.last_error() == "crackle: Invalid range: 0 - 0"
  with pytest.raises(RuntimeError, match=r"^crackle: Invalid range: 0 - 0$"):
    crackle_amd.overlaps(none, none)
  a = checker.compress(np.ones((4, 3, 5), np.uint16, order="F"))
  b = checker.compress(np.ones((4, 3, 5), np.uint64, order="F"), allow_pins=True)
  for z0, z1, msg in ((3, 2, "3 - 2"), (2, 2, "2 - 2"), (9, 4, "4 - 4"), (0, 0, "0 - 0")):
    with pytest.raises(RuntimeError, match=f"^crackle: Invalid range: {msg}$"):
      crackle_amd.overlaps(a, b, z0, z1)
    with pytest.raises(RuntimeError, match=f"^crackle: Invalid range: {msg}$"):
      operations._overlap_counts(a, b, z0, z1)


def test_no_voxels_in_a_slice_gives_an_empty_table(checker):
  a = checker.compress(np.zeros((5, 0, 3), np.uint32, order="F"))
  b = checker.compress(np.zeros((5, 0, 3), np.uint8, order="F"))
  rc, n, p, c = _call(a, b)
  assert rc == _lib.CKL_OK and n == 0 and p and c      # blocks to release even when empty
  assert crackle_amd.overlaps(a, b) == {}
  pairs, counts = operations._overlap_counts(a, b)
  assert pairs.shape == (0, 2) and pairs.dtype == np.uint64 and counts.shape == (0,) and counts.dtype == np.uint64
  assert crackle_amd.CrackleArray(a).overlaps(b) == {}
