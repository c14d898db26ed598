"""GPU tests of contacts (crackle_amd/csrc/ckl_operations.hip: k_run_contacts, k_contacts_compact behind
ckl_decoder_contacts) against the reference's recorded output (tests/golden/contacts.json, see
tests/test_contacts_cpu.py for how it was recorded) and the numpy restatement contacts_numpy, which
tests/test_contacts_cpu.py pins to that output.  Face counts are compared exactly through
ckl_decoder_contacts (crackle_amd.operations._contacts_counts), areas through crackle_amd.contacts
and the pybind module.  contacts always runs the general run pipeline of the decoder; the shapes
below still cover both slice geometries (sx % 4 == 0 with power-of-two rows, odd widths)."""
import hashlib
import json
import os

import numpy as np
import pytest

import contacts_numpy as cn
import crackle_amd
from crackle_amd import _lib, codec, operations, synth
from crackle_amd import fastcrackle as fc
from util import golden

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _fixture():
  with open(os.path.join(HERE, "golden", "contacts.json")) as f:
    return json.load(f)


def _counts(binary, z0=0, z1=-1):
  pairs, faces = operations._contacts_counts(binary, z0, z1)
  assert pairs.shape[0] == 0 or np.all(pairs[:, 0] <= pairs[:, 1])
  keys = [tuple(p) for p in pairs.tolist()]
  assert keys == sorted(keys), "pairs come back ascending by (a, b)"
  return {k: f for k, f in zip(keys, faces.tolist())}


def _same_counts(got, want, what=""):
  assert sorted(got) == sorted(want), what
  for k in want:
    assert list(got[k]) == list(want[k]), (what, k, got[k], want[k])


def test_golden_streams_against_the_reference_fixture(checker):
  """Every golden and signed stream x anisotropy x range: the counts equal contacts_numpy, the areas
  the reference's bit for bit at dyadic weights and within its own rounding otherwise."""
  fx = _fixture()
  want = fx["cases"]
  g = dict(golden())
  inputs = cn.inputs()
  for name, (lab, kw) in cn.signed_volumes().items():
    g[name] = checker.compress(lab, **kw)
    assert hashlib.sha256(g[name]).hexdigest() == fx["streams"][name]
  for name in sorted(g):
    b = g[name]
    lab = inputs[name][0]
    sz = lab.shape[2]
    for rt, z0, z1 in cn.ranges(sz):
      try:
        zs, ze = cn.clamp_range(sz, z0, z1)
      except RuntimeError as exc:
        assert want[cn.case_key(name, "1,1,1", rt)]["error"] == str(exc)
        with pytest.raises(RuntimeError, match="^" + str(exc) + "$"):
          fc.contacts(b, z0, z1, 1.0, 1.0, 1.0)
        continue
      counts = _counts(b, z0, z1)
      _same_counts(counts, cn.contacts_numpy(lab, zs, ze), (name, rt))
      for at, w in cn.ANISOTROPIES.items():
        cn.check_case(want[cn.case_key(name, at, rt)], counts, at)
        got = fc.contacts(b, z0, z1, *w)
        assert got == cn.areas(counts, w), (name, at, rt)
        if rt == "all":
          assert crackle_amd.contacts(b, w) == got, (name, at)


def test_c1_whole_volume_against_its_recorded_digest():
  fx = _fixture()
  lab = cn.c1_volume()
  b = bytes(crackle_amd.compress(lab))
  assert hashlib.sha256(b).hexdigest() == fx["streams"]["c1"]
  w = fx["cases"][cn.case_key("c1", "1,1,1", "all")]
  got = crackle_amd.contacts(b)
  assert len(got) == w["n"] and cn.digest(got) == w["sha256"]


@pytest.mark.parametrize("shape,order", [
  ((128, 64, 9), "F"),      # sx % 4 == 0, power-of-two rows
  ((97, 61, 7), "F"),       # odd widths
  ((96, 80, 6), "C"),       # C order
])
def test_voronoi_against_numpy(checker, shape, order):
  lab = synth.as_numpy_f(synth.voronoi_labels(shape, np.uint32, seed=31, cell=(12, 12, 3)))
  if order == "C":
    lab = np.ascontiguousarray(lab)
  want = cn.contacts_numpy(lab)
  zs = shape[2] // 2
  want_r = cn.contacts_numpy(lab, zs, shape[2])
  for kw in (dict(), dict(allow_pins=True), dict(markov_model_order=5)):
    b = checker.compress(lab, **kw)
    _same_counts(_counts(b), want, kw)
    assert crackle_amd.contacts(b, (4.0, 4.0, 40.0)) == cn.areas(want, (4.0, 4.0, 40.0))
    _same_counts(_counts(b, zs, shape[2]), want_r, (kw, "range"))


def test_c2_sized_voronoi_exact():
  """1024 x 1024 x 512 uint32 Voronoi (the bench volume): every pair's counts equal those taken with
  torch on the device from the labels themselves."""
  import torch
  t = synth.voronoi_labels((1024, 1024, 512), np.uint32, seed=2, cell=(32, 32, 8), device="cuda:0")
  b = crackle_amd.compress(synth.as_numpy_f(t))
  got = _counts(b)
  v = t.view(torch.int32)      # labels below 2^30, shape (z, y, x)
  want = {}
  for axis, dim in ((0, 2), (1, 1), (2, 0)):
    n = v.shape[dim]
    a = v.narrow(dim, 0, n - 1).to(torch.int64)
    c = v.narrow(dim, 1, n - 1).to(torch.int64)
    m = (a != c) & (a != 0) & (c != 0)
    lo, hi = torch.minimum(a[m], c[m]), torch.maximum(a[m], c[m])
    del a, c, m
    keys, cnt = torch.unique(lo * (1 << 31) + hi, return_counts=True)
    for k, n_ in zip(keys.tolist(), cnt.tolist()):
      want.setdefault((k >> 31, k & ((1 << 31) - 1)), [0, 0, 0])[axis] = n_
    del lo, hi, keys, cnt
  assert len(want) > 100000
  _same_counts(got, want)


def test_widths_and_negative_labels(checker):
  for dt in (np.uint8, np.uint16, np.uint32, np.uint64):
    lab = synth.random_labels((31, 29, 5), dt, seed=3, high=9)
    if dt == np.uint64:
      lab = np.asfortranarray(lab + np.uint64(1 << 40))
    b = checker.compress(lab)
    _same_counts(_counts(b), cn.contacts_numpy(lab), np.dtype(dt).name)
  for dt in (np.int8, np.int16, np.int32, np.int64):
    lab = np.asfortranarray((synth.random_labels((31, 29, 5), np.int64, seed=4, high=7) - 3).astype(dt))
    for kw in (dict(), dict(allow_pins=True)):
      b = checker.compress(lab, **kw)
      got = _counts(b)
      _same_counts(got, cn.contacts_numpy(lab), (np.dtype(dt).name, kw))
      assert (2**64 - 3, 2**64 - 1) in got      # -3 and -1, keyed as 2^64 - k
      assert crackle_amd.contacts(b) == cn.areas(got, (1, 1, 1))


def test_pins_with_a_background_colour_outside_the_unique_list(checker):
  lab = synth.as_numpy_f(synth.voronoi_labels((64, 48, 6), np.uint16, seed=5, cell=(8, 8, 2), modulus=40))
  b = bytes(crackle_amd.compress(lab, allow_pins=True, bgcolor=777))
  head = crackle_amd.header(b)
  n, off = codec._label_section(b, head)
  uniq = np.frombuffer(b, dtype=head.stored_dtype, offset=off, count=n).tolist()
  assert head.label_format != crackle_amd.LabelFormat.FLAT and 777 not in uniq
  want = cn.contacts_numpy(lab)
  _same_counts(_counts(b), want)
  b = checker.compress(lab, allow_pins=True, markov_model_order=5)
  _same_counts(_counts(b), want)


def test_degenerate_shapes(checker):
  for shape in ((1, 37, 6), (41, 1, 6), (33, 27, 1), (1, 1, 9), (1, 1, 1)):
    lab = synth.random_labels(shape, np.uint16, seed=6, high=4)
    b = checker.compress(lab)
    want = cn.contacts_numpy(lab)
    _same_counts(_counts(b), want, shape)
    assert fc.contacts(b, 0, -1, 1.0, 1.0, 1.0) == cn.areas(want, (1, 1, 1))
  empty = checker.compress(np.zeros((5, 0, 3), np.uint32, order="F"))
  assert crackle_amd.contacts(empty) == {} and fc.contacts(empty, 0, -1, 1.0, 1.0, 1.0) == {}
  none = checker.compress(np.zeros((0, 0, 0), np.uint8, order="F"))
  with pytest.raises(RuntimeError, match=r"^crackle: Invalid range: 0 - 0$"):
    crackle_amd.contacts(none)
  lab = synth.random_labels((20, 18, 6), np.uint8, seed=7, high=5)
  b = checker.compress(lab)
  with pytest.raises(RuntimeError, match=r"^crackle: Invalid range: 4 - 3$"):
    fc.contacts(b, 4, 3, 1.0, 1.0, 1.0)
  # z_start past the end is clamped to the last slice (src/operations.hpp:878)
  assert fc.contacts(b, 100, -1, 1.0, 1.0, 1.0) == cn.areas(cn.contacts_numpy(lab, 5, 6), (1, 1, 1))


def _floordiv_stream(binary):
  """What the reference's floordiv_scalar(binary, 2) writes for a flat stream: the unique list
  rewritten v // 2 at its stored width, the label-section crc32c fixed, the crack codes unchanged."""
  b = bytearray(binary)
  head = crackle_amd.header(bytes(b))
  n, off = codec._label_section(bytes(b), head)
  uniq = np.frombuffer(bytes(b), dtype=head.stored_dtype, offset=off, count=n)
  b[off:off + uniq.nbytes] = (uniq // 2).astype(head.stored_dtype).tobytes()
  start = head.header_bytes + head.grid_index_bytes
  crc = _lib.lib().ckl_crc32c(bytes(b[start:start + head.num_label_bytes]), head.num_label_bytes)
  at = len(b) - (head.sz * 4 + 4)
  b[at:at + 4] = int(crc).to_bytes(4, "little")
  return bytes(b)


def test_label_merged_stream_reports_self_pairs(checker):
  """Adjacent components that share a label after a label-table rewrite: (a, a) from in-plane faces
  only, pairs that map to 0 dropped."""
  lab = synth.as_numpy_f(synth.voronoi_labels((72, 64, 6), np.uint8, seed=8, cell=(8, 8, 2)))
  b = _floordiv_stream(checker.compress(lab))
  merged = np.asfortranarray(lab // 2)
  want = cn.contacts_numpy(merged, components=lab)
  selfs = [k for k in want if k[0] == k[1]]
  assert selfs and all(want[k][2] == 0 for k in selfs)
  _same_counts(_counts(b), want)
  assert crackle_amd.contacts(b) == cn.areas(want, (1, 1, 1))


def test_many_distinct_pairs():
  """Noise with thousands of labels: a workgroup's 2048 runs bring ~10^4 distinct pairs against the
  1024 entries of its LDS table, and the volume more pairs than the first global table has entries
  (sized for 16 pairs per label: 65536 entries for 3000 labels): both overflow paths run, the
  counts stay exact."""
  lab = synth.random_labels((96, 96, 8), np.uint32, seed=9, high=3000)
  b = crackle_amd.compress(lab)
  want = cn.contacts_numpy(lab)
  assert len(want) > 65536
  _same_counts(_counts(b), want)
  lab = synth.random_labels((128, 128, 4), np.uint16, seed=10, high=60000)
  b = crackle_amd.compress(lab)
  _same_counts(_counts(b), cn.contacts_numpy(lab))


def test_exact_beyond_2_24():
  """4097 x 4096 x 2 uint8, label 1 over label 2: 16 781 312 z faces, area 16781312.0 exactly.  The
  reference's float32 running sum stops at 16777216.0 (2^24 + 1 is not a float32)."""
  lab = np.ones((4097, 4096, 2), np.uint8, order="F")
  lab[:, :, 1] = 2
  b = bytes(crackle_amd.compress(lab))
  assert _counts(b) == {(1, 2): [0, 0, 16781312]}
  assert crackle_amd.contacts(b) == {(1, 2): 16781312.0}
  assert fc.contacts(b, 0, -1, 1.0, 1.0, 1.0) == {(1, 2): 16781312.0}


def test_repeatable():
  """The same stream twice gives the same output: the counts do not depend on the order atomics land."""
  lab = synth.random_labels((80, 72, 6), np.uint32, seed=11, high=2500)
  b = crackle_amd.compress(lab)
  p1, f1 = operations._contacts_counts(b)
  p2, f2 = operations._contacts_counts(b)
  assert np.array_equal(p1, p2) and np.array_equal(f1, f2)


def test_pybind_positional_call_as_the_reference_python():
  """crackle/operations.py:964: fastcrackle.contacts(binary, 0, -1, wx, wy, wz)."""
  lab = synth.as_numpy_f(synth.voronoi_labels((48, 40, 5), np.uint32, seed=12, cell=(8, 8, 2)))
  b = bytes(crackle_amd.compress(lab))
  wx, wy, wz = (0.5, 2.0, 8.0)
  got = fc.contacts(b, 0, -1, wx, wy, wz)
  assert got == crackle_amd.contacts(b, (wx, wy, wz)) == cn.areas(cn.contacts_numpy(lab), (wx, wy, wz))
  assert all(isinstance(k[0], int) and isinstance(v, float) for k, v in got.items())
