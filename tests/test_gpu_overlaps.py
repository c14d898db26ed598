"""GPU tests of overlaps (crackle_amd/csrc/ckl_operations.hip: k_run_overlaps and k_contacts_compact behind
ckl_decoder_overlaps / ckl_overlaps).  The reference has no such function: every case compares the whole
table exactly with the numpy restatement overlaps_numpy (tests/overlaps_numpy.py, pinned by
tests/test_overlaps_cpu.py), taken from the input arrays and never from what the device decodes."""
import ctypes as C

import numpy as np
import pytest

import crackle_amd
from crackle_amd import _lib, operations, synth
from decode_session import DecodeSession
import overlaps_numpy as on

pytestmark = pytest.mark.gpu

S = np.s_


def _as_table(pairs, counts):
  assert pairs.dtype == np.uint64 and counts.dtype == np.uint64
  assert pairs.shape == (counts.shape[0], 2)
  keys = [tuple(p) for p in pairs.tolist()]
  assert keys == sorted(keys) and len(set(keys)) == len(keys), "pairs come back ascending by (a, b), each once"
  return dict(zip(keys, counts.tolist()))


def _table(a, b, z0=0, z1=-1):
  return _as_table(*operations._overlap_counts(a, b, z0, z1))


def _same(got, want, what=""):
  assert sorted(got) == sorted(want), what
  for k in want:
    assert got[k] == want[k], (what, k, got[k], want[k])


def _both_orders(bin_a, bin_b, lab_a, lab_b, what=""):
  want = on.overlaps_numpy(lab_a, lab_b)
  _same(_table(bin_a, bin_b), want, what)
  _same(_table(bin_b, bin_a), on.swapped(want), (what, "swapped"))
  return want


@pytest.mark.parametrize("shape,order_a,order_b", on.GEOMETRY, ids=lambda p: "x".join(map(str, p)) if isinstance(p, tuple) else p)
def test_voronoi_geometries_and_encodings(checker, shape, order_a, order_b):
  lab_a, lab_b = on.geometry_pair(shape, order_a, order_b)
  zs, sz = shape[2] // 2, shape[2]
  want, want_r = on.overlaps_numpy(lab_a, lab_b), on.overlaps_numpy(lab_a, lab_b, zs, sz)
  on.check_partition(want, lab_a, lab_b)
  plain_a, plain_b = checker.compress(lab_a), checker.compress(lab_b)
  cases = [(plain_a, plain_b, "plain")]
  for kw in on.ENCODINGS[1:]:
    cases.append((checker.compress(lab_a, **kw), plain_b, ("A", kw)))
    cases.append((plain_a, checker.compress(lab_b, **kw), ("B", kw)))
  for a, b, what in cases:
    _same(_table(a, b), want, what)
    _same(_table(a, b, zs, sz), want_r, (what, "range"))
  assert crackle_amd.overlaps(plain_a, plain_b) == want
  assert crackle_amd.CrackleArray(plain_a).overlaps(crackle_amd.CrackleArray(plain_b)) == want
  assert crackle_amd.CrackleArray(plain_a).overlaps(plain_b) == want
  assert all(type(k[0]) is int and type(k[1]) is int and type(v) is int for k, v in crackle_amd.overlaps(plain_a, plain_b).items())


def test_both_argument_orders(checker):
  """One run per row against a run per pixel or so, whichever stream the threads run over."""
  lab_a, lab_b = on.one_label_pair()
  want = _both_orders(checker.compress(lab_a), checker.compress(lab_b), lab_a, lab_b)
  assert {k[0] for k in want} == {5} and len(want) == 50


def test_different_crack_formats(checker):
  lab_a, lab_b = on.crack_format_pair()
  a, b = checker.compress(lab_a), checker.compress(lab_b)
  assert crackle_amd.header(a).crack_format != crackle_amd.header(b).crack_format
  _both_orders(a, b, lab_a, lab_b)


def test_widths_and_signs(checker):
  for name, (lab_a, lab_b) in on.unsigned_pairs().items():
    _both_orders(checker.compress(lab_a), checker.compress(lab_b), lab_a, lab_b, name)
  for name, (lab_a, lab_b) in on.signed_pairs().items():
    b = checker.compress(lab_b)
    for kw in (dict(), dict(allow_pins=True)):
      a = checker.compress(lab_a, **kw)
      _both_orders(a, b, lab_a, lab_b, (name, kw))
      assert any(k[0] == 2**64 - 3 for k in _table(a, b))      # -3, keyed as 2^64 - 3


def test_pins_with_a_background_colour_outside_the_unique_list(checker):
  lab_a, lab_b = on.pin_pair()
  a = bytes(crackle_amd.compress(lab_a, allow_pins=True, bgcolor=777))
  head = crackle_amd.header(a)
  n, off = crackle_amd.codec._label_section(a, head)
  uniq = np.frombuffer(a, dtype=head.stored_dtype, offset=off, count=n).tolist()
  assert head.label_format != crackle_amd.LabelFormat.FLAT and 777 not in uniq
  _both_orders(a, checker.compress(lab_b), lab_a, lab_b)
  _both_orders(a, checker.compress(lab_b, allow_pins=True), lab_a, lab_b, "pins on both sides")


def test_identity_and_label_edits(checker):
  lab = on.edit_volume()
  a = checker.compress(lab)
  diag = _table(a, a)
  assert all(k[0] == k[1] for k in diag)
  assert {k[0]: n for k, n in diag.items()} == on.voxel_counts_numpy(lab) == crackle_amd.voxel_counts(a)
  # adjacent components that share a label after a remap: their counts are added, not overwritten
  merged = operations.remap(a, {int(v): int(v) // 4 for v in np.unique(lab)})
  lab_m = np.asfortranarray(lab // 4)
  want = on.overlaps_numpy(lab_m, lab)
  assert len(want) == len(np.unique(lab)) and len({k[0] for k in want}) < len(want)
  _same(_table(merged, a), want, "remap")
  _same(_table(operations.recompress(merged), a), want, "recompress")
  _same(_table(merged, operations.recompress(merged)), on.overlaps_numpy(lab_m, lab_m), "remap against recompress")


def test_paste_changes_pairs_inside_the_box_only(checker):
  lab = on.edit_volume()
  a = checker.compress(lab)
  box = S[10:30, 20:41, 1:4]
  data = synth.random_labels((20, 21, 3), np.uint8, seed=50, high=3) + np.uint8(100)
  edited = lab.copy(order="F")
  edited[box] = data
  got = _table(a, crackle_amd.paste(a, box, data))
  _same(got, on.overlaps_numpy(lab, edited))
  off = {k: n for k, n in got.items() if k[0] != k[1]}
  assert off and all(k[1] in (100, 101, 102) for k in off) and sum(off.values()) == data.size
  outside = np.ones(lab.shape, bool)
  outside[box] = False
  uniq, cnt = np.unique(lab[outside], return_counts=True)
  assert {k[0]: n for k, n in got.items() if k[0] == k[1]} == dict(zip(uniq.tolist(), cnt.tolist()))


def test_many_distinct_pairs():
  """Noise against noise: a workgroup's 2048 runs bring some 2000 distinct pairs against the 1024 entries of its
  LDS table, and the volume more pairs than the first global table has entries (32768 for 3000 labels a side;
  tests/test_overlaps_cpu.py repeats the rule): both overflow paths run, the counts stay exact."""
  lab_a, lab_b = on.many_pairs()
  want = on.overlaps_numpy(lab_a, lab_b)
  assert len(want) > on.first_capacity(3000, 3000) > on.LDS_ENTRIES
  _same(_table(crackle_amd.compress(lab_a), crackle_amd.compress(lab_b)), want)
  lab_a, lab_b = on.many_pairs_mixed_widths()
  _both_orders(crackle_amd.compress(lab_a), crackle_amd.compress(lab_b), lab_a, lab_b)


def test_degenerate_shapes(checker):
  for shape in on.DEGENERATE:
    lab_a, lab_b = on.degenerate_pair(shape)
    _both_orders(checker.compress(lab_a), checker.compress(lab_b), lab_a, lab_b, shape)
  lab_a, lab_b = on.degenerate_pair((20, 18, 6))
  a, b = checker.compress(lab_a), checker.compress(lab_b)
  # z_start past the end is clamped to the last slice, z_end to sz
  _same(_table(a, b, 100, -1), on.overlaps_numpy(lab_a, lab_b, 5, 6))
  _same(_table(a, b, 2, 100), on.overlaps_numpy(lab_a, lab_b, 2, 6))
  with pytest.raises(RuntimeError, match=r"^crackle: Invalid range: 4 - 3$"):
    _table(a, b, 4, 3)


def _flip_a_crack_code_byte(binary, k):
  head = crackle_amd.header(binary)
  hb = head.header_bytes
  lens = np.frombuffer(binary, dtype="<u4", offset=hb, count=head.sz)
  at = hb + head.grid_index_bytes + head.num_label_bytes + head.markov_model_bytes + int(lens[:k].sum())
  assert lens[k] > 8
  bad = bytearray(binary)
  bad[at + int(lens[k]) // 2] ^= 0x04
  return bytes(bad)


def test_damaged_stream(checker):
  """One byte of a crack code of slice 2, in B only and then in A only: what decompress raises for that stream."""
  lab_a, lab_b = on.geometry_pair((64, 48, 6))
  a, b = checker.compress(lab_a), checker.compress(lab_b)
  for good, bad_of in ((a, b), (b, a)):
    bad = _flip_a_crack_code_byte(bad_of, 2)
    with pytest.raises(Exception) as want:
      crackle_amd.decompress(bad)
    assert "z=2" in str(want.value)
    for args in ((good, bad), (bad, good)):
      with pytest.raises(Exception) as got:
        crackle_amd.overlaps(*args)
      assert type(got.value) is type(want.value) and str(got.value) == str(want.value)
    # a range without the slice is not touched by it
    _same(_table(good, bad, 3, 6), on.overlaps_numpy(lab_a, lab_b, 3, 6) if good is a else on.overlaps_numpy(lab_b, lab_a, 3, 6))


def test_repeatable():
  """The same streams twice give the same arrays: the counts do not depend on the order atomics land."""
  lab_a, lab_b = on.repeat_pair()
  a, b = crackle_amd.compress(lab_a), crackle_amd.compress(lab_b)
  p1, c1 = operations._overlap_counts(a, b)
  p2, c2 = operations._overlap_counts(a, b)
  assert np.array_equal(p1, p2) and np.array_equal(c1, c2)
  _same(_as_table(p1, c1), on.overlaps_numpy(lab_a, lab_b))


def test_c1_sized_volume():
  """512 x 512 x 128 uint32, the timing tool's pair (an over-segmentation against a segmentation): the table
  equals the one torch.unique takes from the labels themselves on the device."""
  import torch
  ta, tb = on.timing_pair(on.C1_SHAPE, "cuda:0")
  a = crackle_amd.compress(synth.as_numpy_f(ta))
  b = crackle_amd.compress(synth.as_numpy_f(tb))
  pairs, counts = operations._overlap_counts(a, b)
  va, vb = ta.view(torch.int32).to(torch.int64), tb.view(torch.int32).to(torch.int64)      # labels below 2^31
  keys, cnt = torch.unique(va * (1 << 31) + vb, return_counts=True)
  assert keys.numel() > 10**4
  want_pairs = torch.stack([keys >> 31, keys & ((1 << 31) - 1)], dim=1).cpu().numpy().astype(np.uint64)
  assert np.array_equal(pairs, want_pairs)      # ascending keys are ascending (a, b)
  assert np.array_equal(counts, cnt.cpu().numpy().astype(np.uint64))
  assert int(counts.sum()) == 512 * 512 * 128
  for col, v in ((0, va), (1, vb)):
    lab, n = torch.unique(v, return_counts=True)
    sums = np.zeros(int(lab.numel()), np.uint64)
    idx = np.searchsorted(lab.cpu().numpy().astype(np.uint64), pairs[:, col])
    np.add.at(sums, idx, counts)
    assert np.array_equal(sums, n.cpu().numpy().astype(np.uint64))


# ---- sessions --------------------------------------------------------------------------------------------------------
def _session_overlaps(sa, sb):
  L = _lib.lib()
  pp, cp, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
  try:
    rc = L.ckl_decoder_overlaps(sa.h, sb.h, C.byref(pp), C.byref(cp), C.byref(n))
    if rc != _lib.CKL_OK:
      return rc, _lib.last_error()
    k = int(n.value)
    assert pp.value and cp.value
    if k == 0:
      return rc, {}
    pairs = np.ctypeslib.as_array(C.cast(pp, C.POINTER(C.c_uint64)), shape=(k, 2)).copy()
    counts = np.ctypeslib.as_array(C.cast(cp, C.POINTER(C.c_uint64)), shape=(k,)).copy()
    return rc, _as_table(pairs, counts)
  finally:
    for p in (pp, cp):
      if p.value:
        L.ckl_free(p)


def _span_ms(sess):
  ms, gvox = C.c_float(), C.c_float()
  assert _lib.lib().ckl_decoder_last_timing(sess.h, C.byref(ms), C.byref(gvox)) == _lib.CKL_OK
  return ms.value


def test_sessions_in_every_order(checker):
  lab_a, lab_b = on.session_pair()
  a, b = checker.compress(lab_a), checker.compress(lab_b, markov_model_order=5)
  want = on.overlaps_numpy(lab_a, lab_b)
  vol_a, vol_b = crackle_amd.decompress(a), crackle_amd.decompress(b)
  assert np.array_equal(vol_a, lab_a) and np.array_equal(vol_b, lab_b)
  # overlaps, then a full run of each session
  with DecodeSession(a) as sa, DecodeSession(b) as sb:
    rc, got = _session_overlaps(sa, sb)
    assert rc == _lib.CKL_OK
    _same(got, want, "overlaps first")
    assert _span_ms(sa) > 0
    assert np.array_equal(sa.run(), vol_a) and np.array_equal(sb.run(), vol_b)
    # twice, and with the sessions swapped
    _same(_session_overlaps(sa, sb)[1], want, "again")
    _same(_session_overlaps(sb, sa)[1], on.swapped(want), "swapped")
    assert _span_ms(sb) > 0
    # one session against itself
    _same(_session_overlaps(sa, sa)[1], on.overlaps_numpy(lab_a, lab_a), "itself")
  # a run first (the strip path's paint builds no run tables), then overlaps
  with DecodeSession(a) as sa, DecodeSession(b) as sb:
    assert np.array_equal(sa.run(), vol_a) and np.array_equal(sb.run(), vol_b)
    _same(_session_overlaps(sa, sb)[1], want, "run first")
    _same(_session_overlaps(sa, sb)[1], want, "run first, again")
    assert np.array_equal(sb.run(), vol_b) and np.array_equal(sa.run(), vol_a)


def test_sessions_on_different_ranges(checker):
  lab_a, lab_b = on.session_pair()
  a, b = checker.compress(lab_a), checker.compress(lab_b)
  # equal lengths: slice i of the one against slice i of the other
  with DecodeSession(a, 1, 4) as sa, DecodeSession(b, 5, 8) as sb:
    rc, got = _session_overlaps(sa, sb)
    assert rc == _lib.CKL_OK
    _same(got, on.overlaps_numpy(lab_a[:, :, 1:4], lab_b[:, :, 5:8]))
  with DecodeSession(a, 0, 4) as sa, DecodeSession(b, 0, 5) as sb:
    rc, msg = _session_overlaps(sa, sb)
    assert rc == _lib.CKL_ERR_ARG and "4 slices" in msg and "5 slices" in msg
    # both remain usable
    assert np.array_equal(sa.run(), lab_a[:, :, 0:4]) and np.array_equal(sb.run(), lab_b[:, :, 0:5])
  other = checker.compress(np.ones((64, 40, 8), np.uint8, order="F"))
  with DecodeSession(a) as sa, DecodeSession(other) as sb:
    rc, msg = _session_overlaps(sa, sb)
    assert rc == _lib.CKL_ERR_ARG and "64 x 48" in msg and "64 x 40" in msg
