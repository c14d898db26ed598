"""k_trail_emit (crackle_amd/csrc/ckl_encode.hip): from the trail's items to the packed crack codes in one workgroup
per slice, the code points OR-ed into words in LDS at their final index (ckl_code_words.hpp), against the three
kernels it stands in for (k_trail_offsets + k_trail_expand + k_finish: CKL_TRAIL_EMIT=0, or an LDS cap below what
the largest slice asks for: CKL_TRAIL_EMIT_LDS), and against itself with a word buffer of four words, so that every
slice is emitted in windows (CKL_TRAIL_EMIT_WORDS).

Every case compares the encoder's bytes with the checker's on each of the four settings and decodes them again.
The volumes are built in numpy so that what a case is about holds by construction; where that is a code index
(alignment in a word, a slice's total), the case sweeps one dimension over 16 consecutive sizes instead: the crack's
topology stays, so the index moves by one per size and takes every residue mod 16, whatever the chain's constant
share of control codes is."""
import numpy as np
import pytest
import torch

import crackle_amd
from crackle_amd import distributed as ckd
from crackle_amd import synth
from test_gpu_trail_long_segments import RECTS, crack_graph, first_vertex, many_components, notch, single_path

pytestmark = pytest.mark.gpu

INLINE = 64      # kInlineCodes: longer segments are walked again, shorter ones shifted into place from their dart's 16 bytes

# the settings every case runs on: environment, does k_trail_emit run
SETTINGS = [
  ("k_trail_emit", {}, True),
  ("three kernels forced", {"CKL_TRAIL_EMIT": "0"}, False),
  ("LDS cap forces the three kernels", {"CKL_TRAIL_EMIT_LDS": "4096"}, False),
  ("k_trail_emit in windows of 4 words", {"CKL_TRAIL_EMIT_WORDS": "4"}, True),
]


def device_volume(arr):
  return torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 1, 0))).to("cuda:0")


def slice_index(binary, z):
  """(start vertices (x, y) of slice z's chains as its beginning-of-chain index lists them, bytes of its packed codes):
  read from a stream, so that a case can assert what the reference made of its volume (write_boc_index,
  crackcodes.hpp:318-372; the payload holds 4 code points per byte)."""
  h = crackle_amd.header(binary)
  hb = h.header_bytes
  assert h.markov_model_order == 0
  lens = [int.from_bytes(binary[hb + 4 * k:hb + 4 * k + 4], "little") for k in range(h.sz)]
  off = hb + h.grid_index_bytes + h.num_label_bytes + sum(lens[:z])
  sec = binary[off:off + lens[z]]
  width = lambda v: 1 if v < 256 else (2 if v < 65536 else 4)
  xw, yw = width(h.sx + 1), width(h.sy + 1)
  size = int.from_bytes(sec[:4], "little")
  p = 4
  num_y = int.from_bytes(sec[p:p + yw], "little"); p += yw
  starts, y = [], 0
  for _ in range(num_y):
    y += int.from_bytes(sec[p:p + yw], "little"); p += yw
    n = int.from_bytes(sec[p:p + xw], "little"); p += xw
    x = 0
    for _ in range(n):
      x += int.from_bytes(sec[p:p + xw], "little"); p += xw
      starts.append((x, y))
  assert p == 4 + size
  return starts, lens[z] - 4 - size


def every_setting(arr, checker, monkeypatch, **kw):
  """The checker's bytes from crackle_amd.compress and from a HipBackend session on every setting; the session's
  emit_path() confirms which kernels ran (uint8 volumes only: they go to the device as they are).  One round trip: the
  bytes are the same."""
  assert arr.dtype == np.uint8
  want = checker.compress(arr, **kw)
  be = ckd.HipBackend(0)
  for name, env, fused in SETTINGS:
    for k, v in env.items():
      monkeypatch.setenv(k, v)
    try:
      got = crackle_amd.compress(arr, **kw)
      via = be.encode(device_volume(arr), arr.shape, markov_model_order=kw.get("markov_model_order", 0))
      path = be.emit_path()[0]
    finally:
      for k in env:
        monkeypatch.delenv(k)
    assert got == want, (name, arr.shape, kw)
    assert via == want, (name, arr.shape, kw)
    assert path == fused, (name, arr.shape)
  back = crackle_amd.decompress(want)
  assert back.dtype == arr.dtype and np.array_equal(back, arr), (arr.shape, kw)
  return want


# ---- segment lengths around the inline limit and the word size
LENGTHS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1000]


@pytest.mark.parametrize("length", LENGTHS)
def test_straight_segment(length, checker, monkeypatch):
  """Two half-planes: one crack straight down the slice, `length` moves between two dead ends on the border."""
  arr = np.ones((12, length, 2), np.uint8, order="F")
  arr[7:, :, :] = 2
  single_path(arr, length)
  every_setting(arr, checker, monkeypatch)


@pytest.mark.parametrize("length", LENGTHS)
def test_staircase_segment(length, checker, monkeypatch):
  """The same with one step sideways (the step is one of the `length` moves).  A crack of one move has no room for
  a step: that length runs on the two-move staircase's slice shape with the step at the border, i.e. straight."""
  sy = max(length - 1, 1)
  arr = np.ones((12, sy, 2), np.uint8, order="F")
  if length == 1:
    arr[7:, :, :] = 2
  else:
    arr[7:, : sy // 2, :] = 2
    arr[8:, sy // 2:, :] = 2
  single_path(arr, length)
  every_setting(arr, checker, monkeypatch)


# ---- every alignment of an item in a word, every residue of a slice's total
def stripes(sx, n_cracks):
  """n_cracks straight cracks of sx moves across the slice, border to border, three rows apart: each is a chain of its own
  (two dead ends), and they come in start-vertex order."""
  arr = np.ones((sx, 3 * n_cracks + 3, 1), np.uint8, order="F")
  for j in range(n_cracks):
    arr[:, 3 * j + 3:, 0] = j + 2
  return arr


@pytest.mark.parametrize("sx0", [17, 49, 65], ids=["inline-short", "inline-up-to-64", "walked"])
def test_every_alignment_and_total(sx0, checker, monkeypatch):
  """Three cracks of sx moves each: the second and third chain begin where the chains in front end, at (sx + c) and
  2 (sx + c) code points, c the chain's control codes; the slice's total is 3 (sx + c).  Over 16 consecutive sx the
  second chain's first item starts at every position of a word and the total takes every residue mod 16 (3 is odd):
  totals of 16 k - 1, 16 k, 16 k + 1 and the byte tails 4 k + 1 .. 4 k + 3 are among them.  sx <= 64: the items are
  shifted in from the darts' 16 bytes (up to five words); above, they are walked.
  Asserted from the reference's streams: the three chains start where the cracks meet the left border, in that order,
  and the packed codes grow by exactly 3 bytes = 12 code points per 4 more pixels of width from every sx on, which only
  a total of 3 sx + constant gives: all 16 residues of the total (and of the second chain's start, a third of it)."""
  payload = {}
  for sx in range(sx0, sx0 + 16):
    arr = stripes(sx, 3)
    deg, edges = crack_graph(arr[:, :, 0])
    assert edges == 3 * sx and int((deg == 1).sum()) == 6 and int((deg > 2).sum()) == 0
    assert (sx <= INLINE) == (sx0 < 65)
    want = every_setting(arr, checker, monkeypatch)
    starts, payload[sx] = slice_index(want, 0)
    assert starts == [(0, 3), (0, 6), (0, 9)]
  assert all(payload[sx + 4] - payload[sx] == 3 for sx in range(sx0, sx0 + 12))
  assert {payload[sx] % 4 for sx in payload} == {0, 1, 2, 3}


def test_alignment_of_items_inside_a_chain(checker, monkeypatch):
  """Nodes along one chain: a comb of walls of growing length hangs from one crack, so the chain's segment and
  control items follow each other at every alignment (segment lengths 1 .. 20 in one chain, 'b' and 't' between)."""
  arr = np.ones((90, 30, 2), np.uint8, order="F")
  arr[:, 4:, :] = 2
  for j in range(20):
    arr[4 * j + 2, 4:5 + j, :] = 3 + j
  every_setting(arr, checker, monkeypatch)


# ---- chains
def test_isolated_components_land_in_start_vertex_order(checker, monkeypatch):
  """20 x 15 isolated pixels, every one a closed loop and a chain of its own, and a block whose top-left corner lies in
  front of them all although its loop is the longest.  (Loops start at their own smallest vertex: the chains are in
  start-vertex order as they come; test_moved_start_lands_behind_a_later_chain is the case that permutes.)"""
  arr = np.zeros((64, 48, 2), np.uint8, order="F")
  xs, ys = np.meshgrid(np.arange(3, 43, 2), np.arange(5, 35, 2), indexing="ij")
  for z in range(2):
    arr[xs, ys, z] = 1 + (xs + ys) % 200
  arr[1:60, 1:3, :] = 250
  deg, _ = crack_graph(arr[:, :, 0])
  assert int(((deg != 0) & (deg != 2)).sum()) == 0, "closed loops only"
  assert first_vertex(deg) == (1, 1)
  every_setting(arr, checker, monkeypatch)


def test_first_chain_begins_with_a_branch(checker, monkeypatch):
  """The slice's first crack vertex is the top-left corner of a block that a wall divides: the trail leaves it with a
  'b', the component has nodes (the wall's two T junctions) and the start splits a segment.  The branch is not an
  initial one to remove (another 'b' follows before its 't'): the reference keeps the start where it is."""
  arr = np.ones((40, 30, 2), np.uint8, order="F")
  arr[4:30, 3:20, :] = 2
  arr[12:30, 3:20, :] = 3
  arr[33:36, 25:28, 1] = 9
  deg, _ = crack_graph(arr[:, :, 0])
  assert first_vertex(deg) == (4, 3) and deg[4, 3] == 2
  assert int((deg == 3).sum()) == 2
  want = every_setting(arr, checker, monkeypatch)
  assert slice_index(want, 0)[0] == [(4, 3)]


def test_moved_start_lands_behind_a_later_chain(checker, monkeypatch):
  """An open crack with one corner: from the corner (10, 5), its smallest vertex, right, down a step and right to the
  border; and down to the bottom border.  The trail leaves the corner with a 'b' and meets a dead end without another
  branch: remove_initial_branch (crackcodes.hpp:185-242) reverses that stretch and moves the chain's start to the border
  vertex (40, 9).  An isolated pixel at (25, 6) lies between the two: its chain comes second (chains come out by their
  components' smallest vertices) and must land first.  The reference's index says so."""
  arr = np.ones((40, 30, 2), np.uint8, order="F")
  arr[10:20, 5:, :] = 2
  arr[20:, 9:, :] = 2
  arr[25, 6, :] = 9
  deg, _ = crack_graph(arr[:, :, 0])
  assert first_vertex(deg) == (10, 5) and deg[10, 5] == 2, "the open crack's corner is the slice's first crack vertex"
  assert 5 * 41 + 10 < 6 * 41 + 25 < 9 * 41 + 40
  want = every_setting(arr, checker, monkeypatch)
  for z in range(2):
    assert slice_index(want, z)[0] == [(25, 6), (40, 9)]


def test_more_walked_segments_than_the_list_holds(checker, monkeypatch):
  """1100 straight cracks of 65 moves in one slice: more segments to walk than k_trail_emit lists (kEmitLong = 1024), so
  it has no walking wavefronts and every thread walks the long segments it meets."""
  n = 1100
  arr = np.ones((INLINE + 1, 3 * n + 3, 1), np.uint8, order="F")
  for j in range(n):
    arr[:, 3 * j + 3:, 0] = 2 + j % 250
  deg, edges = crack_graph(arr[:, :, 0])
  assert edges == n * (INLINE + 1) and int((deg == 1).sum()) == 2 * n and int((deg > 2).sum()) == 0
  assert n > 1024
  every_setting(arr, checker, monkeypatch)


@pytest.mark.parametrize("perimeter", sorted(RECTS))
@pytest.mark.parametrize("nested", [False, True], ids=["single", "nested"])
def test_closed_loops_without_nodes(perimeter, nested, checker, monkeypatch):
  w, h = RECTS[perimeter]
  arr = np.ones((w + 9, h + 10, 2), np.uint8, order="F")
  if nested:
    arr[2:w + 6, 3:h + 7, :] = 5
  arr[4:w + 4, 5:h + 5, :] = 9
  for z in range(2):
    deg, _ = crack_graph(arr[:, :, z])
    assert int(((deg != 0) & (deg != 2)).sum()) == 0, "no vertex is a node"
  every_setting(arr, checker, monkeypatch)


def test_more_chains_than_the_staged_tables_hold(checker, monkeypatch):
  """2836 closed loops in one slice: more chains than k_trail_emit stages in LDS (2048, as k_finish), so its chain
  tables stay in global memory.  (The labels taken mod 250: the loops stay apart, the background keeps them so.)"""
  big = many_components()
  arr = np.where(big > 0, big % 250 + 1, 0).astype(np.uint8, order="F")
  deg, _ = crack_graph(arr[:, :, 0])
  assert np.array_equal(deg, crack_graph(big[:, :, 0])[0])
  assert 63 * 45 + 1 > 2048
  every_setting(arr, checker, monkeypatch)


def test_start_vertex_inside_a_long_segment(checker, monkeypatch):
  arr = notch(sx=80, a=40, b=50, t=5, y1=65, sy=70)
  single_path(arr, 200)
  every_setting(arr, checker, monkeypatch)


# ---- empty and trivial slices
def test_empty_and_trivial_slices(checker, monkeypatch):
  flat = np.full((40, 70, 3), 7, np.uint8, order="F")
  assert crack_graph(flat[:, :, 0])[1] == 0
  every_setting(flat, checker, monkeypatch)
  one_slice = np.ones((12, 130, 1), np.uint8, order="F")
  one_slice[7:, :, :] = 2
  single_path(one_slice, 130)
  every_setting(one_slice, checker, monkeypatch)
  between = np.full((33, 21, 3), 4, np.uint8, order="F")
  between[5:20, 6:11, 1] = 8
  between[20:25, 6:18, 1] = 9
  assert [crack_graph(between[:, :, z])[1] > 0 for z in range(3)] == [False, True, False]
  every_setting(between, checker, monkeypatch)
  pixel = np.full((1, 1, 1), 3, np.uint8, order="F")
  every_setting(pixel, checker, monkeypatch)


# ---- markov models, reencode
@pytest.fixture(scope="module")
def long_mix():
  """Slices with a 200-move open crack, a notch (start inside a segment), a loop of 400 and short pieces."""
  arr = np.ones((200, 160, 3), np.uint8, order="F")
  arr[:, 120:, :] = 2
  arr[40:50, 30:120, :] = 2
  arr[60:160, 5:105, 0] = 3
  arr[100:130, 10:20, 1] = 4
  arr[150:170, 60:130, 2] = 5
  for z in range(3):
    assert crack_graph(arr[:, :, z])[1] > 3 * INLINE
  return arr


@pytest.mark.parametrize("order", [1, 5])
def test_markov_models(long_mix, order, checker, monkeypatch):
  every_setting(long_mix, checker, monkeypatch, markov_model_order=order)


def test_reencode(long_mix, checker, monkeypatch):
  b0 = checker.compress(long_mix)
  b5 = checker.compress(long_mix, markov_model_order=5)
  for name, env, _ in SETTINGS:
    for k, v in env.items():
      monkeypatch.setenv(k, v)
    try:
      got5 = crackle_amd.reencode(b0, 5)
      got0 = crackle_amd.reencode(b5, 0)
    finally:
      for k in env:
        monkeypatch.delenv(k)
    assert got5 == b5 and got0 == b0, name
  assert np.array_equal(crackle_amd.decompress(b5), long_mix)


# ---- the decision between the two paths
def test_fallback_decision_at_the_lds_cap(long_mix, checker, monkeypatch):
  """The same volume with the cap at what its largest slice asks for, and one byte below: k_trail_emit, then the three
  kernels, the same bytes.  Without a cap the volume is far below the default one."""
  want = checker.compress(long_mix)
  vol = device_volume(long_mix)
  be = ckd.HipBackend(0)
  assert be.encode(vol, long_mix.shape) == want
  fused, need = be.emit_path()
  assert fused and 0 < need < 80 * 1024
  for cap, expect in ((need, True), (need - 1, False), (need + 1, True), (0, False)):
    monkeypatch.setenv("CKL_TRAIL_EMIT_LDS", str(cap))
    try:
      got = be.encode(vol, long_mix.shape)
      path = be.emit_path()
    finally:
      monkeypatch.delenv("CKL_TRAIL_EMIT_LDS")
    assert got == want, cap
    assert path == (expect, need), cap


def test_oversized_slices_take_the_three_kernels(checker):
  """Binary noise, 512 x 512: a quarter of a million crack edges per slice, whose words would take more LDS than two
  workgroups per CU leave (80 KiB).  No switch is set: emit_plan itself hands the volume to the three kernels."""
  vol = synth.random_labels_device((512, 512, 2), np.uint8, seed=4, high=2, device="cuda:0")
  arr = np.asfortranarray(synth.as_numpy_f(vol))
  assert min(crack_graph(arr[:, :, z])[1] for z in range(2)) > 200000
  be = ckd.HipBackend(0)
  got = be.encode(vol, arr.shape)
  fused, need = be.emit_path()
  assert not fused and need > 80 * 1024
  assert got == checker.compress(arr)
  assert np.array_equal(crackle_amd.decompress(got), arr)


def test_mixed_random_volume(checker, monkeypatch):
  arr = synth.as_numpy_f(synth.voronoi_labels((257, 130, 3), np.uint8, seed=43, cell=(24, 24, 2)))
  every_setting(np.asfortranarray(arr), checker, monkeypatch)
