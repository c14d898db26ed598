"""Crack segments on both sides of what the trail keeps beside a dart (kInlineCodes = 64 code points,
crackle_amd/csrc/ckl_trail.hpp): longer segments, closed loops without a node and the halves of a segment that
k_trail_components splits at a chain's start vertex are the ones k_trail_expand walks again instead of copying;
slices with more chains than kStartList, and the three placements of k_trail_components' tables (LDS, union-find
table in LDS with the minima in global memory, both global).
Every volume is built in numpy so that the length, the loop, the start vertex or the component count it is about
holds by construction (asserted here from the array's geometry); every case compares the encoder's bytes with the
checker's and decodes them again."""
import numpy as np
import pytest

import crackle_amd
from crackle_amd import synth
from cc3d_numpy import connected_components

pytestmark = pytest.mark.gpu

INLINE = 64          # kInlineCodes
START_LIST = 2048    # kStartList: more chains than this in a slice are ranked by the bitmap scan


def crack_graph(sl):
  """(degree of every crack vertex [sx + 1, sy + 1], crack edges) of one slice whose cracks run between differing
  pixels (crackcodes.hpp:66-125); vertex (x, y) is the top-left corner of pixel (x, y)."""
  sx, sy = sl.shape
  deg = np.zeros((sx + 1, sy + 1), np.int64)
  v = sl[1:, :] != sl[:-1, :]        # edge from vertex (i + 1, y) to (i + 1, y + 1)
  deg[1:sx, :sy] += v
  deg[1:sx, 1:] += v
  h = sl[:, 1:] != sl[:, :-1]        # edge from vertex (x, j + 1) to (x + 1, j + 1)
  deg[:sx, 1:sy] += h
  deg[1:, 1:sy] += h
  return deg, int(v.sum() + h.sum())


def first_vertex(deg):
  """Smallest vertex index y * (sx + 1) + x that carries a crack, as (x, y)."""
  ys, xs = np.nonzero(deg.T)
  return int(xs[0]), int(ys[0])


def same_bytes_and_back(arr, checker, **kw):
  want = checker.compress(arr, **kw)
  got = crackle_amd.compress(arr, **kw)
  assert got == want, (arr.shape, kw)
  back = crackle_amd.decompress(got)
  assert back.dtype == arr.dtype and np.array_equal(back, arr), (arr.shape, kw)
  return got


def single_path(arr, length):
  """Every slice of arr holds exactly one open crack of `length` moves between two dead ends."""
  for z in range(arr.shape[2]):
    deg, edges = crack_graph(arr[:, :, z])
    assert edges == length, (edges, length)
    assert int((deg == 1).sum()) == 2 and int((deg > 2).sum()) == 0
    assert int((deg == 2).sum()) == length - 1


# ---- one open segment on both sides of the threshold
@pytest.mark.parametrize("length", [63, 64, 65, 130])
def test_straight_segment_at_the_inline_length(length, checker):
  """Two half-planes: one crack straight down the volume, `length` moves between two dead ends on the border."""
  arr = np.ones((12, length, 2), np.uint8, order="F")
  arr[7:, :, :] = 2
  single_path(arr, length)
  assert (length <= INLINE) == (length in (63, 64))
  same_bytes_and_back(arr, checker)


@pytest.mark.parametrize("length", [63, 64, 65, 130])
def test_staircase_segment_at_the_inline_length(length, checker):
  """The same with one step sideways in the middle (the step is one of the `length` moves)."""
  sy = length - 1
  arr = np.ones((12, sy, 2), np.uint8, order="F")
  arr[7:, : sy // 2, :] = 2
  arr[8:, sy // 2:, :] = 2
  single_path(arr, length)
  same_bytes_and_back(arr, checker)


def test_very_long_segment(checker):
  """1024 x 8 x 2 split along x: one crack of 1024 moves, both ends of degree 1 on the border."""
  arr = np.ones((1024, 8, 2), np.uint16, order="F")
  arr[:, 4:, :] = 300
  single_path(arr, 1024)
  same_bytes_and_back(arr, checker)


# ---- closed loops without a node (k_trail_loops)
RECTS = {60: (10, 20), 64: (12, 20), 68: (14, 20), 400: (100, 100)}


@pytest.mark.parametrize("perimeter", sorted(RECTS))
@pytest.mark.parametrize("nested", [False, True], ids=["single", "nested"])
def test_closed_loops_without_nodes(perimeter, nested, checker):
  w, h = RECTS[perimeter]
  arr = np.ones((w + 9, h + 10, 2), np.uint8, order="F")
  if nested:
    arr[2:w + 6, 3:h + 7, :] = 5      # a loop around the loop, two pixels away
  arr[4:w + 4, 5:h + 5, :] = 9
  for z in range(2):
    deg, edges = crack_graph(arr[:, :, z])
    assert int(((deg != 0) & (deg != 2)).sum()) == 0, "no vertex is a node"
    assert edges == perimeter + (2 * (w + 4 + h + 4) if nested else 0)
  _, comps = connected_components(arr, 6)
  assert len(comps) == (3 if nested else 2)
  same_bytes_and_back(arr, checker)


# ---- a chain's start vertex inside a long segment (the split in k_trail_components)
def notch(sx, a, b, t, y1, sy):
  """Label 2 below row y1 and in the columns a .. b - 1 above it, from row t on: one open crack from the left border
  along y1, up column a, along row t, down column b, on along y1 to the right border.  Its smallest vertex is the
  corner (a, t): a + (y1 - t) moves from the left end, (b - a) + (y1 - t) + (sx - b) from the right end."""
  arr = np.ones((sx, sy, 2), np.uint8, order="F")
  arr[:, y1:, :] = 2
  arr[a:b, t:y1, :] = 2
  return arr


@pytest.mark.parametrize("left,right,geom", [
  (10, 200, dict(sx=198, a=4, b=9, t=3, y1=9, sy=12)),
  (64, 65, dict(sx=61, a=30, b=40, t=2, y1=36, sy=40)),
  (100, 100, dict(sx=80, a=40, b=50, t=5, y1=65, sy=70)),
], ids=["10+200", "64+65", "100+100"])
def test_start_vertex_inside_a_long_segment(left, right, geom, checker):
  arr = notch(**geom)
  a, b, t, y1, sx = geom["a"], geom["b"], geom["t"], geom["y1"], geom["sx"]
  assert a + (y1 - t) == left and (b - a) + (y1 - t) + (sx - b) == right
  single_path(arr, left + right)
  deg, _ = crack_graph(arr[:, :, 0])
  assert first_vertex(deg) == (a, t) and deg[a, t] == 2, "the chain starts at a vertex of degree 2, inside the segment"
  assert deg[0, y1] == 1 and deg[sx, y1] == 1
  same_bytes_and_back(arr, checker)


# ---- many components in one slice
def many_components():
  arr = np.zeros((128, 128, 1), np.uint16, order="F")
  xs, ys = np.meshgrid(np.arange(1, 127, 2), np.arange(1, 91, 2), indexing="ij")
  arr[xs, ys, 0] = (1 + (xs // 2 + 64 * (ys // 2))).astype(np.uint16)      # 63 x 45 isolated pixels off the border, every one its own label
  arr[10:60, 95:120, 0] = 60000      # a rectangle of perimeter 150
  return arr


@pytest.fixture(scope="module")
def many(checker):
  arr = many_components()
  deg, _ = crack_graph(arr[:, :, 0])
  assert int(((deg != 0) & (deg != 2)).sum()) == 0, "closed loops only"
  _, comps = connected_components(arr, 6)
  assert len(comps) == 63 * 45 + 1 and len(comps) > START_LIST      # (the background is label 0: not counted)
  assert 2 * (50 + 25) > INLINE
  return arr, checker.compress(arr)


def test_many_components_bitmap_ranking(many):
  arr, want = many
  assert crackle_amd.compress(arr) == want
  assert np.array_equal(crackle_amd.decompress(want), arr)


@pytest.mark.parametrize("lds,tables", [("4096", "both global"), ("16384", "union-find in LDS, minima global")], ids=["global", "mixed"])
def test_many_components_table_placements(many, lds, tables, monkeypatch):
  """2836 loop nodes: 12 bytes per node (34032) fit neither size, 4 bytes per node (11344) fit 16384 but not 4096."""
  arr, want = many
  nodes = 63 * 45 + 1
  assert 12 * nodes > int(lds) and (4 * nodes <= int(lds)) == (tables != "both global")
  monkeypatch.setenv("CKL_TRAIL_LDS", lds)
  try:
    got = crackle_amd.compress(arr)
    back = crackle_amd.decompress(got)
  finally:
    monkeypatch.delenv("CKL_TRAIL_LDS")
  assert got == want, tables
  assert back.dtype == arr.dtype and np.array_equal(back, arr), tables


# ---- long segments under other settings
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
    deg, edges = crack_graph(arr[:, :, z])
    assert edges > 3 * INLINE
  return arr


def test_long_segments_with_a_markov_model(long_mix, checker):
  same_bytes_and_back(long_mix, checker, markov_model_order=3)


@pytest.mark.parametrize("walk", ["plain", "lds"])
def test_long_segments_under_the_other_walks(long_mix, walk, checker, monkeypatch):
  monkeypatch.setenv("CKL_TRAIL_WALK", walk)
  try:
    same_bytes_and_back(long_mix, checker)
  finally:
    monkeypatch.delenv("CKL_TRAIL_WALK")


def test_long_segments_through_reencode(long_mix, checker):
  b0 = same_bytes_and_back(long_mix, checker)
  b5 = crackle_amd.reencode(b0, 5)
  assert b5 == checker.compress(long_mix, markov_model_order=5)
  assert np.array_equal(crackle_amd.decompress(b5), long_mix)
  assert crackle_amd.reencode(b5, 0) == b0


# ---- thin volumes and no crack at all
def test_thin_volumes(checker):
  one_slice = np.ones((12, 130, 1), np.uint8, order="F")
  one_slice[7:, :, :] = 2
  single_path(one_slice, 130)
  same_bytes_and_back(one_slice, checker)
  column = np.ones((1, 200, 2), np.uint8, order="F")
  column[:, 100:, :] = 2
  for z in range(2):
    deg, edges = crack_graph(column[:, :, z])
    assert edges == 1 and int((deg == 1).sum()) == 2
  same_bytes_and_back(column, checker)
  flat = np.full((40, 70, 3), 7, np.uint32, order="F")
  assert crack_graph(flat[:, :, 0])[1] == 0
  same_bytes_and_back(flat, checker)


def test_mixed_random_volume(checker):
  arr = synth.as_numpy_f(synth.voronoi_labels((256, 192, 4), np.uint16, seed=41, cell=(48, 48, 2)))
  same_bytes_and_back(arr, checker)
