"""Every kind of stream the library accepts or produces (tests/stream_kinds.py) through every operation, and every
ordered pair of the seven editors.  One pytest parameter is one kind through all operations.  Every comparison is
exact and against an answer that does not come from the code under test: numpy on the volume the kind must decode to
(the restatements tests/*_numpy.py for the editors), or the checker on the same stream for what depends on the
stream's cracks (voxel_connectivity_graph, point_cloud, mode_pooling_2x2x1, reencode).

A cell is one (kind, operation).  REFUSALS names the only cells that may raise: the limits the docstrings state.
Every other cell compares a result; one that raises fails the kind.  All cells of a kind run before the kind fails,
so one run shows every cell that is wrong."""
import functools
import traceback

import numpy as np
import pytest

import cc3d_numpy
import contacts_numpy as cn
import crackle_amd
import dust_numpy
import erode_numpy
import fill_holes_numpy
import overlaps_numpy as on
import paste_volumes
import recompress_volumes as rv
import stream_kinds as sk
from crackle_amd import LabelFormat, operations as ops

pytestmark = pytest.mark.gpu

KINDS = sk.HOST_KINDS + sk.DEVICE_KINDS + sk.LARGE_KINDS
# kinds whose streams hold in-plane neighbours with one label: contacts reports pairs (a, a) for them
MERGED = {"remapped", "floordiv", "permuted-merged", "zsplit-tail", "restacked", "filled", "dusted-filled", "pasted", "large-remapped"}

REFUSALS = {
  ("v0", "connected_components"): (ValueError, "version 0"),
  ("v0", "dust"): (ValueError, "version 0"),
  ("v0", "fill_holes"): (ValueError, "version 0"),
  ("v0", "remap"): (ValueError, "version 0"),
  ("v0", "mask"): (ValueError, "version 0"),
  ("v0", "mask_except"): (ValueError, "version 0"),
  ("v0", "zsplit"): (ValueError, "version 1"),      # "needs version 1 streams"
  ("v0", "zstack"): (ValueError, "version 1"),
  ("pins", "remap"): (ValueError, "pin label"),
  ("pins", "mask"): (ValueError, "pin label"),
  ("pins", "mask_except"): (ValueError, "pin label"),
  ("pins", "zsplit"): (ValueError, "FLAT label streams only"),
  ("pins", "zstack"): (ValueError, "FLAT label streams only"),
  # every pooled slice is compressed on its own and picks its own crack format; the noise of two labels gives
  # slices of both formats, which zstack cannot join (the reference: "All crack formats must match.")
  ("large-remapped", "mode_pooling"): (ValueError, "crack format"),
}


@functools.lru_cache(maxsize=None)
def _checker():
  from oracle import oracle
  return oracle.best()


@functools.lru_cache(maxsize=None)
def _kinds():
  chk = _checker()
  a = sk.volume_a()
  return {k.name: k for k in sk.kinds_host(a, chk) + sk.kinds_device(a, chk) + sk.kinds_large(chk, device=True)}


def _same(got, want):
  assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
  assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()


class Cells:
  """The cells of one kind.  b is the stream, D the volume it must decode to."""

  def __init__(self, kind):
    self.k, self.chk = kind, _checker()
    self.b, self.D = kind.stream, kind.expected
    self.head = crackle_amd.header(self.b)
    self.m = self.head.markov_model_order
    self.sz = self.D.shape[2]
    self.box = sk.box_of(self.D.shape)
    self.inner = (1, self.sz - 1) if self.sz > 2 else (0, self.sz)
    self.stats = sk.stats_numpy(self.D)
    nonzero = {l: s[0] for l, s in self.stats.items() if l != 0}
    self.L = max(nonzero, key=lambda l: (nonzero[l], -l))      # present, not everywhere
    assert 0 < nonzero[self.L] < self.D.size
    self.absent = int(self.D.max()) + 1

  def decoded(self, stream, want):
    """The stream decodes to `want`, by the checker and by this library."""
    _same(sk.decode(self.chk, stream), want)
    got = crackle_amd.decompress(stream)
    _same(got, want)
    assert got.flags.f_contiguous == want.flags.f_contiguous or 1 in want.shape

  def compress(self, vol):
    return self.chk.compress(sk.like(self.D, vol), markov_model_order=self.m)

  # ---- readers --------------------------------------------------------------------------------------------------------
  def decompress(self):
    self.decoded(self.b, self.D)

  def decompress_label(self):
    img = crackle_amd.decompress(self.b, label=self.L)
    _same(img, self.D == self.L)
    assert img.any() and not img.all()
    _same(crackle_amd.decompress(self.b, label=self.absent), np.zeros(self.D.shape, bool))
    if 0 in self.stats:
      _same(crackle_amd.decompress(self.b, label=0), self.D == 0)

  def decompress_range(self):
    z0, z1 = self.inner
    _same(crackle_amd.decompress_range(self.b, z0, z1), self.D[:, :, z0:z1])
    _same(crackle_amd.decompress_range(self.b, z0, z1, label=self.L), self.D[:, :, z0:z1] == self.L)

  def cutout(self):
    _same(crackle_amd.cutout(self.b, self.box), self.D[self.box])
    idx = np.s_[3:40:2, 7, ...]
    _same(crackle_amd.cutout(self.b, idx), self.D[idx])

  def cutout_label(self):
    _same(crackle_amd.cutout(self.b, self.box, label=self.L), self.D[self.box] == self.L)
    _same(crackle_amd.cutout(self.b, self.box, label=self.absent), np.zeros(self.D[self.box].shape, bool))

  def crackle_array(self):
    arr = crackle_amd.CrackleArray(self.b)
    assert arr.shape == self.D.shape and arr.dtype == self.D.dtype
    _same(arr[self.box], self.D[self.box])
    _same(arr[:, :, self.sz - 1], self.D[:, :, self.sz - 1])
    assert self.L in arr and self.absent not in arr
    assert arr.min() == int(self.D.min()) and arr.max() == int(self.D.max())

  def voxel_counts(self):
    want = {l: s[0] for l, s in self.stats.items()}
    assert crackle_amd.voxel_counts(self.b) == want
    assert crackle_amd.voxel_counts(self.b, label=self.L) == want[self.L]
    assert self.chk.voxel_counts(self.b) == want

  def centroids(self):
    want = {l: s[1].astype(np.float64) / np.float64(s[0]) for l, s in self.stats.items()}
    got = crackle_amd.centroids(self.b)
    ref = self.chk.centroids(self.b)
    assert sorted(got) == sorted(want) == sorted(ref)
    for l in want:
      assert got[l].dtype == np.float64 and np.array_equal(got[l], want[l]) and np.array_equal(got[l], ref[l]), l
    assert np.array_equal(crackle_amd.centroids(self.b, label=self.L), want[self.L])

  def bounding_boxes(self):
    """numpy's boxes, with the reference's two rules (src/operations.hpp:541-618): a label of the list that no voxel
    carries keeps the initial box, and a pin stream's background colour outside the list has its minima at 0."""
    want = {l: list(s[2]) for l, s in self.stats.items()}
    listed = set(sk.stored_list(self.b).tolist())
    for l in listed - set(want):
      want[l] = [0xFFFFFFFF] * 3 + [0] * 3
    if self.head.label_format != LabelFormat.FLAT:
      for l in set(want) - listed:
        want[l] = [0, 0, 0] + want[l][3:]
    got = {l: [int(v) for v in box] for l, box in crackle_amd.bounding_boxes(self.b, no_slice_conversion=True).items()}
    assert got == want
    assert {l: [int(v) for v in box] for l, box in self.chk.bounding_boxes(self.b).items()} == want
    x0, y0, z0, x1, y1, z1 = want[self.L]
    assert crackle_amd.bounding_boxes(self.b, label=self.L) == (slice(x0, x1 + 1), slice(y0, y1 + 1), slice(z0, z1 + 1))

  def contacts(self):
    cc2d = self.chk.connected_components(np.asfortranarray(self.k.cracks))[0]
    counts = cn.contacts_numpy(self.D, components=cc2d)
    assert counts or self.k.name == "eroded"      # (every label eroded by 6 is surrounded by 0, which contacts leaves out)
    assert any(a == b for a, b in counts) == (self.k.name in MERGED)
    for aniso in ((1.0, 1.0, 1.0), (4.0, 4.0, 40.0)):
      assert crackle_amd.contacts(self.b, anisotropy=aniso) == cn.areas(counts, aniso), aniso

  def overlaps_other(self):
    o = self.chk.compress(self.k.other)
    want = on.overlaps_numpy(self.D, self.k.other)
    assert crackle_amd.overlaps(self.b, o) == want
    assert crackle_amd.overlaps(o, self.b) == on.swapped(want)
    z0, z1 = self.inner
    assert crackle_amd.overlaps(self.b, o, z0, z1) == on.overlaps_numpy(self.D, self.k.other, z0, z1)

  def overlaps_self(self):
    got = crackle_amd.overlaps(self.b, self.b)
    assert got == {(l, l): s[0] for l, s in self.stats.items()}
    assert {a: n for (a, _), n in got.items()} == crackle_amd.voxel_counts(self.b)

  def overlaps_source(self):
    assert crackle_amd.overlaps(self.b, self.k.source) == on.overlaps_numpy(self.D, self.k.base)
    assert crackle_amd.overlaps(self.k.source, self.b) == on.overlaps_numpy(self.k.base, self.D)

  def _vcg(self, connectivity):
    got = crackle_amd.voxel_connectivity_graph(self.b, connectivity)
    want = self.chk.voxel_connectivity_graph(self.b, connectivity)
    assert got.dtype == np.uint8 and got.flags.f_contiguous
    _same(got, want)
    return got

  def vcg4(self):
    got = self._vcg(4)
    # the +x bit: set where the neighbour lies in the same 2D component of the volume the cracks were made from
    cc2d = self.chk.connected_components(np.asfortranarray(self.k.cracks))[0]
    assert np.array_equal((got[:-1] & 1) != 0, cc2d[:-1] == cc2d[1:])

  def vcg6(self):
    got = self._vcg(6)
    if self.sz > 1:
      assert np.array_equal((got[:, :, :-1] & 0x10) != 0, self.D[:, :, :-1] == self.D[:, :, 1:])

  def point_cloud(self):
    want = self.chk.point_cloud(self.b, 0, -1, None, True)
    got = crackle_amd.point_cloud(self.b)
    assert sorted(got) == sorted(want) == sorted(l for l in self.stats if l != 0)
    for l in want:
      assert got[l].dtype == np.uint16 and got[l].shape[1] == 3 and np.array_equal(got[l].ravel(), want[l]), l
    one = crackle_amd.point_cloud(self.b, self.L)
    assert np.array_equal(one.ravel(), self.chk.point_cloud(self.b, 0, self.sz, [self.L], True)[self.L])
    # every point lies on a voxel of the label or next to one
    x, y, z = (one[:, i].astype(np.int64) for i in range(3))
    assert (z < self.sz).all() and len(one) > 0

  def mode_pooling(self):
    want = self.chk.mode_pooling_2x2x1(self.b)
    assert ops._mode_pooling_slices(self.b) == want
    pooled = crackle_amd.mode_pooling_2x2x1(self.b)
    sx, sy, _ = self.D.shape
    slices = [sk.decode(self.chk, s) for s in want]
    stacked = np.concatenate(slices, axis=2)
    assert stacked.shape == ((sx + 1) // 2, (sy + 1) // 2, self.sz)
    assert np.array_equal(sk.decode(self.chk, pooled), stacked)
    # where the four pixels of a window agree the pooled pixel is theirs, whatever the rule does elsewhere
    ex, ey = sx // 2 * 2, sy // 2 * 2
    a, b, c, d = (np.asarray(self.D)[i:ex:2, j:ey:2] for i, j in ((0, 0), (1, 0), (0, 1), (1, 1)))
    agree = (a == b) & (a == c) & (a == d)
    assert agree.any() and np.array_equal(stacked[:ex // 2, :ey // 2][agree], a[agree])

  def reencode(self):
    other_order = 3 if self.m != 3 else 0
    got = crackle_amd.reencode(self.b, other_order)
    want = self.chk.reencode(self.b, other_order)
    if self.head.format_version == 0:
      # the reference leaves five stray zero bytes behind a version 0 header (tests/test_v0_streams.py)
      assert want[24:29] == b"\x00" * 5
      want = want[:24] + want[29:]
    assert got == want
    assert crackle_amd.header(got).markov_model_order == other_order
    self.decoded(got, self.D)
    assert crackle_amd.reencode(self.b, self.m) == self.b

  def array_equal(self):
    assert crackle_amd.array_equal(self.b, self.chk.compress(self.D))
    assert crackle_amd.array_equal(self.chk.compress(self.D), self.b)
    assert not crackle_amd.array_equal(self.b, self.chk.compress(self.k.other))
    # one voxel given another label of the same volume: the label sets agree, the arrays do not
    at = tuple(np.argwhere(self.D != self.L)[len(self.D) // 2])
    near = self.D.copy(order="K")
    near[at] = self.L
    assert set(np.unique(near).tolist()) == set(np.unique(self.D).tolist()) or self.stats[int(self.D[at])][0] == 1
    assert not crackle_amd.array_equal(self.b, self.chk.compress(near))
    assert not crackle_amd.array_equal(self.chk.compress(near), self.b)
    # two labels exchanged: the same cracks and the same label set, another array
    m = next(l for l in sorted(self.stats, reverse=True) if l != self.L)
    exchanged = sk.like(self.D, np.where(self.D == self.L, m, np.where(self.D == m, self.L, self.D)).astype(self.D.dtype))
    assert not crackle_amd.array_equal(self.b, self.chk.compress(exchanged))
    assert crackle_amd.array_equal(self.chk.compress(exchanged), self.chk.compress(exchanged, markov_model_order=2))

  def structure_equal(self):
    assert crackle_amd.structure_equal(self.b, self.b)
    assert crackle_amd.structure_equal(self.b, self.k.source) == self.k.keeps
    assert crackle_amd.structure_equal(self.k.source, self.b) == self.k.keeps
    assert crackle_amd.structure_equal(self.b, self.compress(self.k.cracks))
    assert not crackle_amd.structure_equal(self.b, self.chk.compress(self.k.other))

  def ok_check(self):
    assert crackle_amd.ok(self.b)
    rep = crackle_amd.check(self.b)
    if self.head.format_version == 0:
      assert rep == {"header": True, "crack_index": True, "labels": None, "z": None}
    else:
      assert rep == {"header": True, "crack_index": True, "labels": True, "z": []}

  # ---- editors --------------------------------------------------------------------------------------------------------
  def recompress(self):
    assert crackle_amd.recompress(self.b) == self.compress(self.D)
    assert crackle_amd.recompress(self.b, markov_model_order=2) == self.chk.compress(self.D, markov_model_order=2)

  def erode(self):
    for connectivity in (6, 26):
      for border in (True, False):
        want = erode_numpy.erode(self.D, connectivity, border)
        assert crackle_amd.erode(self.b, connectivity, erode_border=border) == self.compress(want), (connectivity, border)

  def dust(self):
    for kw in (dict(connectivity=26), dict(connectivity=6, binary_image=True), dict(connectivity=26, invert=True)):
      got, removed = crackle_amd.dust(self.b, sk.DUST[0], return_removed=True, **kw)
      want, n = dust_numpy.dust(self.D, sk.DUST[0], **kw)
      assert removed == n, kw
      self.decoded(got, want)
      head = crackle_amd.header(got)
      assert head.is_sorted and head.label_format == LabelFormat.FLAT and head.data_width == self.head.data_width
      assert np.array_equal(sk.stored_list(got), np.unique(want)), kw
      if "binary_image" not in kw and "invert" not in kw:
        assert crackle_amd.recompress(got) == self.compress(want)

  def fill_holes(self):
    for connectivity in (6, 26):
      got, filled = crackle_amd.fill_holes(self.b, connectivity, return_filled=True)
      want = fill_holes_numpy.fill_holes(self.D, connectivity)
      assert filled == want.filled, connectivity
      self.decoded(got, want.volume)
      head = crackle_amd.header(got)
      assert head.is_sorted and head.label_format == LabelFormat.FLAT
      assert np.array_equal(sk.stored_list(got), np.unique(want.volume)), connectivity
      if connectivity == sk.FILL:
        assert crackle_amd.recompress(got) == self.compress(want.volume)

  def connected_components(self):
    for connectivity in (26, 6):
      got, mapping = crackle_amd.connected_components(self.b, connectivity, return_mapping=True)
      ccl, want_mapping = cc3d_numpy.connected_components(self.D, connectivity)
      want = sk.like(self.D, ccl)
      assert mapping == want_mapping, connectivity
      self.decoded(got, want)
      assert crackle_amd.header(got).data_width == 4
      if connectivity == sk.COMPONENTS:
        assert crackle_amd.recompress(got) == self.compress(want)

  def paste(self):
    data = self.k.other[self.box]
    self.decoded(crackle_amd.paste(self.b, self.box, data), paste_volumes.edited(self.D, self.box, data))
    whole = np.s_[5:60:3, 2, :]      # a stepped x, an int y, the whole depth
    self.decoded(crackle_amd.paste(self.b, whole, 7), paste_volumes.edited(self.D, whole, 7))

  def _edited(self, got, want):
    self.decoded(got, want)
    head = crackle_amd.header(got)
    assert head.is_sorted and head.label_format == LabelFormat.FLAT
    assert np.array_equal(sk.stored_list(got), np.unique(want))
    held = set(np.unique(want).tolist())
    for v in sorted(held | {v + 1 for v in held} | {max(v - 1, 0) for v in held}):      # (labels run to 2^30: no range over them)
      assert crackle_amd.contains(got, v) == (v in held), v

  def remap(self):
    self._edited(crackle_amd.remap(self.b, rv.floordiv_mapping(self.D, 2)), sk.np_remap(self.D))

  def mask(self):
    self._edited(crackle_amd.mask(self.b, [self.L, self.absent]), sk.like(self.D, np.where(self.D == self.L, 0, self.D).astype(self.D.dtype)))

  def mask_except(self):
    self._edited(crackle_amd.mask_except(self.b, [self.L, self.absent], value=3),
                 sk.like(self.D, np.where(self.D == self.L, self.D, 3).astype(self.D.dtype)))

  def zsplit(self):
    z = self.sz // 2
    parts = crackle_amd.zsplit(self.b, z)
    wants = (self.D[:, :, :z], self.D[:, :, z:z + 1], self.D[:, :, z + 1:])
    for part, want in zip(parts, wants):
      if want.shape[2] == 0:
        assert part == b""
      else:
        self.decoded(part, sk.like(self.D, want))
        assert crackle_amd.header(part).is_sorted == self.head.is_sorted
    self.decoded(crackle_amd.zstack([p for p in parts if p]), self.D)
    shards = crackle_amd.zshatter(self.b)
    assert len(shards) == self.sz
    self.decoded(crackle_amd.zstack(shards), self.D)

  def zstack(self):
    twice = sk.like(self.D, np.concatenate([self.D, self.D], axis=2))
    got = crackle_amd.zstack([self.b, self.b])
    self.decoded(got, twice)
    assert (np.diff(sk.stored_list(got).astype(np.int64)) > 0).all()


OPERATIONS = [
  "decompress", "decompress_label", "decompress_range", "cutout", "cutout_label", "crackle_array",
  "voxel_counts", "centroids", "bounding_boxes", "contacts", "overlaps_other", "overlaps_self", "overlaps_source",
  "vcg4", "vcg6", "point_cloud", "mode_pooling", "reencode", "array_equal", "structure_equal", "ok_check",
  "recompress", "erode", "dust", "fill_holes", "connected_components", "paste", "remap", "mask", "mask_except",
  "zsplit", "zstack",
]
TALLY = {}


def test_the_refusal_table_names_kinds_and_operations():
  assert all(kind in KINDS and op in OPERATIONS for kind, op in REFUSALS)
  assert len(OPERATIONS) == len(set(OPERATIONS)) == 32 and len(KINDS) == len(set(KINDS)) == 22
  assert all(callable(getattr(Cells, op)) for op in OPERATIONS)


@pytest.mark.parametrize("name", KINDS)
def test_every_operation_on_the_kind(name):
  kind = _kinds()[name]
  _same(sk.decode(_checker(), kind.stream), kind.expected)
  cells = Cells(kind)
  compared, refused, failures = 0, 0, []
  for op in OPERATIONS:
    refusal = REFUSALS.get((name, op))
    try:
      if refusal is not None:
        with pytest.raises(refusal[0], match=refusal[1]):
          getattr(cells, op)()
        refused += 1
      else:
        getattr(cells, op)()
        compared += 1
    except BaseException as e:      # pytest.raises' own failure included: every cell runs, every wrong one is named
      if isinstance(e, KeyboardInterrupt):
        raise
      failures.append(f"{name} x {op}: {type(e).__name__}: {e}\n{traceback.format_exc(limit=-3)}")
      print(failures[-1], flush=True)
  TALLY[name] = (compared, refused)
  print(f"{name}: {compared} cells compared, {refused} refused")
  assert not failures, "\n".join(failures)
  assert refused == sum(1 for kind_name, _ in REFUSALS if kind_name == name)
  assert compared == len(OPERATIONS) - refused


# ---- editor after editor ------------------------------------------------------------------------------------------------

def _box_data(vol):
  box = sk.box_of(vol.shape)
  return box, sk.other_of(vol)[box]


# name: (the editor on a stream whose volume is V, the same in numpy)
EDITORS = {
  "remap": (lambda b, V: crackle_amd.remap(b, rv.floordiv_mapping(V, 2)), sk.np_remap),
  "dust": (lambda b, V: crackle_amd.dust(b, sk.DUST[0], connectivity=sk.DUST[1]), sk.np_dust),
  "fill_holes": (lambda b, V: crackle_amd.fill_holes(b, sk.FILL), sk.np_fill),
  "connected_components": (lambda b, V: crackle_amd.connected_components(b, sk.COMPONENTS), sk.np_components),
  "paste": (lambda b, V: crackle_amd.paste(b, *_box_data(V)), sk.np_paste),
  "erode": (lambda b, V: crackle_amd.erode(b, sk.ERODE[0], erode_border=sk.ERODE[1]), sk.np_erode),
  "recompress": (lambda b, V: crackle_amd.recompress(b), sk.np_recompress),
}
# (first, second) where the second editor documents that it returns its input's bytes when it changes nothing
SAME_BYTES = {("dust", "dust"), ("fill_holes", "fill_holes"), ("recompress", "recompress"), ("erode", "recompress")}
PAIRS = {}


@pytest.mark.parametrize("first", list(EDITORS))
def test_every_editor_after_the_editor(first):
  chk = _checker()
  V0 = sk.volume_a8() if first == "connected_components" else sk.volume_a()
  b0 = chk.compress(V0)
  device1, numpy1 = EDITORS[first]
  b1, V1 = device1(b0, V0), numpy1(V0)
  _same(sk.decode(chk, b1), V1)
  assert not np.array_equal(V1, V0) or first == "recompress"
  failures, done = [], 0
  for second, (device2, numpy2) in EDITORS.items():
    try:
      b2, V2 = device2(b1, V1), numpy2(V1)
      _same(sk.decode(chk, b2), V2)
      _same(crackle_amd.decompress(b2), V2)
      assert crackle_amd.recompress(b2) == chk.compress(V2)
      assert crackle_amd.ok(b2)
      if (first, second) in SAME_BYTES:
        assert np.array_equal(V2, V1) and b2 == b1
      done += 1
    except Exception as e:
      failures.append(f"{second} after {first}: {type(e).__name__}: {e}\n{traceback.format_exc(limit=-3)}")
      print(failures[-1], flush=True)
  PAIRS[first] = done
  print(f"after {first}: {done} pairs compared")
  assert not failures, "\n".join(failures)
  assert done == len(EDITORS) == 7


def test_the_cell_count():
  """kinds x operations - refusals cells and 49 pairs: counted from what ran in this process when the whole module
  ran, and from the tables in any case."""
  want = len(KINDS) * len(OPERATIONS) - len(REFUSALS)
  assert want == 22 * 32 - 14
  for name, (compared, refused) in TALLY.items():
    assert compared + refused == len(OPERATIONS)
  if len(TALLY) == len(KINDS):
    assert sum(c for c, _ in TALLY.values()) == want
  if len(PAIRS) == len(EDITORS):
    assert sum(PAIRS.values()) == 49
  print(f"cells compared: {sum(c for c, _ in TALLY.values())} of {want}; refusals: {sum(r for _, r in TALLY.values())} of {len(REFUSALS)}; "
        f"editor pairs: {sum(PAIRS.values())} of 49")
