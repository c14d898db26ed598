"""Pins the constructions of tests/threshold_volumes.py against the checker, on the CPU: every volume that
tests/test_gpu_volume_reductions.py and tests/test_gpu_sharded.py run through the kernels must sit where it is meant
to sit (this many pairs, this crack and label format, this stored width in the checker's own stream).  A case that
stops reaching its edge fails here instead of quietly covering nothing.

The wrap-around bound.  A count that forgets the pairs across row and slice wrap-arounds finds pairs_in_rows.  For
the strip shapes and the sharded volume that is below H - 1 (H = voxels // 2) for every k of {H - 1, H, H + 1}: with
the wraps forgotten every one of these volumes, the IMPERMISSIBLE ones too, comes out PERMISSIBLE.  The small shapes
cannot reach that bound: a stretch of at most H + 2 voxels of a (17, 3, 1), (48, 5, 1) or (40, 5, 1) slice holds the
starts of one or two rows only, so pairs_in_rows = k - 1 or k - 2.  There the wraps are counted (at least one in
every case) and the case that decides, k = H, must come out below H without them."""
import numpy as np
import pytest

import crackle_amd
import threshold_volumes as tv


def _names(dtype, shape):
  return f"{np.dtype(dtype).name}-{'x'.join(map(str, shape))}"


def _head(checker, arr, **kw):
  return crackle_amd.header(checker.compress(arr, **kw))


def _check_formats(checker, arr, k):
  h = arr.size // 2
  sz = arr.shape[2] if arr.ndim == 3 else 1
  assert tv.pairs(arr) == k
  head = _head(checker, arr)
  assert (head.crack_format == tv.PERMISSIBLE) == (k < h), (k, h)
  assert head.label_format == tv.FLAT
  assert head.stored_data_width == tv.byte_width(int(arr.max()))
  pins = _head(checker, arr, allow_pins=True)
  assert (pins.crack_format == tv.PERMISSIBLE) == (k < h), (k, h)
  assert (pins.label_format == tv.PINS) == (k >= h and sz > 1), (k, h, sz)
  assert pins.label_format in (tv.FLAT, tv.PINS)
  assert pins.stored_data_width == tv.byte_width(int(arr.max()))


STATS_CASES = [(dt, shape) for dt in tv.DTYPES for shape in tv.all_shapes(dt)]


@pytest.mark.parametrize("dtype,shape", STATS_CASES, ids=[_names(*c) for c in STATS_CASES])
def test_pairs_volumes_sit_on_the_threshold(dtype, shape, checker):
  """Every pairs_volume of the reductions test (a) and of the format test (b)."""
  n = shape[0] * shape[1] * shape[2]
  h = n // 2
  ks = tv.threshold_ks(shape)
  assert ks, shape
  if n >= 4:
    assert ks == [h - 1, h, h + 1]
  for k in ks:
    for place in ("head", "tail"):
      arr = tv.pairs_volume(shape, dtype, k, place)
      assert arr.dtype == dtype and arr.shape == shape and arr.flags.f_contiguous
      _check_formats(checker, arr, k)
      # the stretch covers the volume's midpoint (both placements meet there) and, beyond one row, a wrap-around
      f = tv.flat(arr)
      assert f[0 if place == "head" else -1] == 3
      assert f[h - 1 if place == "head" else n - h] == 3, (k, place)
      if shape in tv.strip_shapes(dtype):
        assert tv.pairs_in_rows(arr) < h - 1, (k, place)
        # row wraps and both slice wraps lie inside a stretch of half the volume, whichever end it starts from
        assert tv.wraps_in_rows(arr) >= shape[1] * shape[2] // 2 - 1
        sxy = shape[0] * shape[1]
        assert f[sxy - 1] == f[sxy] == 3 if place == "head" else f[2 * sxy - 1] == f[2 * sxy] == 3
      elif shape == (17, 3, 1):
        assert tv.wraps_in_rows(arr) == 1, (k, place)
        if k == h:
          assert tv.pairs_in_rows(arr) < h
      # the same volume with the dtype's maximum in its first and last voxel (test a)
      ext = tv.with_extremes(arr)
      top = int(np.iinfo(dtype).max)
      assert int(tv.flat(ext)[0]) == int(tv.flat(ext)[-1]) == top == int(ext.max())
      assert _head(checker, ext).stored_data_width == np.dtype(dtype).itemsize


def test_odd_voxel_count_rounds_the_threshold_down(checker):
  """51 voxels: 25 pairs are not fewer than 51 // 2 = 25, though they are fewer than 51 / 2."""
  arr = tv.pairs_volume((17, 3, 1), np.uint8, 25, "tail")
  assert arr.size == 51 and tv.pairs(arr) == 25
  assert _head(checker, arr).crack_format == tv.IMPERMISSIBLE
  assert _head(checker, tv.pairs_volume((17, 3, 1), np.uint8, 24, "tail")).crack_format == tv.PERMISSIBLE


def test_random_volumes_are_not_all_on_one_side():
  """The seeded random volumes of test a: labels below 3, so that pairs are frequent and the count is a large number
  that a lost strip, band or wrap changes."""
  for dt in tv.DTYPES:
    for shape in tv.all_shapes(dt):
      arr = tv.random_volume(shape, dt)
      assert arr.dtype == dt and arr.shape == shape and arr.flags.f_contiguous
      if shape in tv.strip_shapes(dt):
        assert tv.pairs(arr) > arr.size // 4
        assert tv.wraps_in_rows(arr) > 0


MAX_CASES = [(dt, value, width, shape) for dt, value, width in tv.MAX_VALUES for shape in tv.strip_shapes(dt)]


@pytest.mark.parametrize("dtype,value,width,shape", MAX_CASES, ids=[f"{_names(c[0], c[3])}-{c[1]}" for c in MAX_CASES])
def test_max_at_holds_one_wide_voxel(dtype, value, width, shape, checker):
  assert width == tv.byte_width(value)
  p = tv.lanes(dtype)
  where = tv.max_positions(shape, dtype)
  assert set(where) == set(tv.POSITIONS)
  assert where["strip_end"][0] == 64 * p - 1 and where["strip_next"][0] == 64 * p < shape[0]
  assert where["y31"][1] == 31 and where["y32"][1] == 32 == shape[1] - 1
  seen = set()
  for position in tv.POSITIONS:
    arr = tv.max_at(shape, dtype, value, position)
    assert arr.dtype == dtype and arr.shape == shape and arr.flags.f_contiguous
    at = np.argwhere(arr > 3)
    assert at.shape == (1, 3) and tuple(at[0]) == where[position], position
    seen.add(tuple(at[0]))
    assert int(arr[where[position]]) == value == int(arr.max())
    assert _head(checker, arr).stored_data_width == width, position
  assert len(seen) == len(tv.POSITIONS)
  f = tv.flat(tv.max_at(shape, dtype, value, "slice1"))
  assert int(f[shape[0] * shape[1]]) == value


POOL_CASES = [(dt, w) for dt in tv.DTYPES for w in tv.POOL_WIDTHS]


@pytest.mark.parametrize("dtype,width", POOL_CASES, ids=[f"{np.dtype(d).name}-{w}" for d, w in POOL_CASES])
def test_pooling_input_pools_to_the_threshold_slices(dtype, width, checker):
  slices = tv.pooling_slices(width, dtype)
  h = width * 5 // 2
  for s, k in zip(slices, (h - 1, h, h + 1)):
    assert s.shape == (width, 5)
    vol = s.reshape(width, 5, 1)
    assert tv.pairs(vol) == k
    assert tv.wraps_in_rows(vol) == 2
    if k == h:
      assert tv.pairs_in_rows(vol) < h
    assert (_head(checker, np.asfortranarray(vol)).crack_format == tv.PERMISSIBLE) == (k < h)
  big = tv.pooling_input(width, dtype)
  assert big.shape == (2 * width, 10, 3) and big.dtype == dtype and big.flags.f_contiguous
  for z, s in enumerate(slices):
    for dx in (0, 1):
      for dy in (0, 1):
        assert np.array_equal(big[dx::2, dy::2, z], s)      # every 2 x 2 block holds one value: its mode is that value
  pooled = checker.mode_pooling_2x2x1(checker.compress(big))
  assert pooled == [checker.compress(np.asfortranarray(s.reshape(width, 5, 1))) for s in slices]
  # the second width's uint8 slices start at byte offsets that are no multiple of 16
  assert (tv.POOL_WIDTHS[1] * 5 * np.dtype(np.uint8).itemsize) % 16 != 0


def test_sharded_volumes_cross_the_slab_boundary(checker):
  sx, sy, sz = tv.SHARDED_SHAPE
  n = sx * sy * sz
  h = n // 2
  at, below = tv.sharded_volume(h), tv.sharded_volume(h - 1)
  _check_formats(checker, at, h)
  _check_formats(checker, below, h - 1)
  for arr in (at, below):
    assert tv.pairs_in_rows(arr) < h - 1
  # two slabs of two slices: the stretch of H + 1 voxels begins with the first slab's last voxel, so the pair that
  # straddles the slabs is one of the H; without it the slabs' sums give H - 1, the other format
  f = tv.flat(at)
  assert f[n // 2 - 1] == f[n // 2] == 3 and f[n // 2 - 2] != 3
  slabs = [at[:, :, :2], at[:, :, 2:]]
  assert sum(tv.pairs(np.asfortranarray(s)) for s in slabs) == h - 1
  g = tv.flat(below)
  assert g[n // 2] == 3 and g[n // 2 - 1] != 3
  assert sum(tv.pairs(np.asfortranarray(s)) for s in (below[:, :, :2], below[:, :, 2:])) == h - 1
