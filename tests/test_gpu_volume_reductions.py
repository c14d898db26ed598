"""The encoder's two whole-volume reductions, pixel_pairs and max_label, where they decide the stream's shape: volumes
with exactly H - 1, H and H + 1 equal linear neighbours (H = voxels // 2: the crack format changes at H) and volumes
whose one wide label sits where a strip, a band or a slice of the planes kernel begins or ends (the stored width).
tests/threshold_volumes.py builds them; tests/test_threshold_volumes_cpu.py pins them against the checker.

The shapes reach both kernels.  With P labels to a 16-byte vector, (65 P, 33, 3) runs k_label_planes_stream with one
full strip and a strip of one lane, one full band and a band of one row; (65 P + 1, 33, 3), (P - 1, 2, 2) and
(17, 3, 1) run k_stats; (P, 1, 1) is the smallest volume of the fast kernel.  A view that starts one element into a
buffer runs k_stats on every shape.  Everything is compared exactly."""
import numpy as np
import pytest
import torch

import crackle_amd
from crackle_amd import distributed as ckd
from crackle_amd import operations

import threshold_volumes as tv
from oracle_backend import OracleBackend

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIGNED = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}


def _name(dtype, shape):
  return f"{np.dtype(dtype).name}-{'x'.join(map(str, shape))}"


def _aligned(arr):
  """The volume on the device, x fastest, at a 16-byte aligned address."""
  t = torch.from_numpy(tv.flat(arr).view(SIGNED[arr.dtype.itemsize])).to(DEV)
  assert t.data_ptr() % 16 == 0
  return t


def _unaligned(arr):
  """The same voxels as a view that starts one element into a larger buffer: never 16-byte aligned, and for uint8 and
  uint16 the first and the last voxel share their 4-byte words with the buffer's other elements."""
  t = _aligned(arr)
  buf = torch.full((t.numel() + 16,), -1 if arr.dtype.itemsize > 1 else 255, dtype=t.dtype, device=DEV)
  view = buf[1:1 + t.numel()]
  view.copy_(t)
  assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == arr.dtype.itemsize
  return view


def _takes_fast_path(shape, dtype):
  p = tv.lanes(dtype)
  return shape[0] >= p and shape[0] % p == 0


# ---- a. the reductions themselves -----------------------------------------------------------------------------------
def _stats_volumes(shape, dtype):
  """(name, volume): the threshold volumes, two of them and the noise also with the dtype's maximum at both ends."""
  h = shape[0] * shape[1] * shape[2] // 2
  out = []
  for k in tv.threshold_ks(shape):
    for place in ("head", "tail"):
      arr = tv.pairs_volume(shape, dtype, k, place)
      out.append((f"k={k} {place}", arr))
      if k == min(h, arr.size - 1):
        out.append((f"k={k} {place} extremes", tv.with_extremes(arr)))
  noise = tv.random_volume(shape, dtype)
  out.append(("noise", noise))
  out.append(("noise extremes", tv.with_extremes(noise)))
  return out


STATS_CASES = [(dt, shape) for dt in tv.DTYPES for shape in tv.all_shapes(dt)]


@pytest.mark.parametrize("dtype,shape", STATS_CASES, ids=[_name(*c) for c in STATS_CASES])
def test_stats_equal_numpy_and_oracle(dtype, shape):
  p = tv.lanes(dtype)
  assert _takes_fast_path(shape, dtype) == (shape in ((65 * p, 33, 3), (p, 1, 1)))
  be, oracle = ckd.HipBackend(0), OracleBackend()
  top = int(np.iinfo(dtype).max)
  volumes = _stats_volumes(shape, dtype)
  assert any(int(tv.flat(a)[0]) == top and int(tv.flat(a)[-1]) == top for _, a in volumes)
  for name, arr in volumes:
    f = tv.flat(arr)
    want = (int(arr.max()), tv.pairs(arr), int(f[0]), int(f[-1]))
    assert oracle.stats(arr, shape) == want, (name, "oracle")
    for how, make in (("aligned", _aligned), ("unaligned", _unaligned)):
      t = make(arr)
      got = be.stats(t, shape)
      print(f"{_name(dtype, shape)} {name} {how}: max, pairs, first, last = {got}, numpy {want}")
      assert got == want, (name, how)
      del t


# ---- b. the format decision -----------------------------------------------------------------------------------------
FORMAT_CASES = [(dt, shape, kw) for dt in tv.DTYPES for shape in tv.format_shapes(dt)
                for kw in [dict(), dict(allow_pins=True)] + ([dict(markov_model_order=3)] if dt in (np.uint8, np.uint32) else [])]


def _kw_name(kw):
  return "pins" if kw.get("allow_pins") else f"m{kw['markov_model_order']}" if kw.get("markov_model_order") else "flat"


@pytest.mark.parametrize("dtype,shape,kw", FORMAT_CASES, ids=[f"{_name(c[0], c[1])}-{_kw_name(c[2])}" for c in FORMAT_CASES])
def test_format_decision_at_half_the_voxels(dtype, shape, kw, checker):
  """k = H - 1 is the last PERMISSIBLE volume, k = H the first IMPERMISSIBLE one (with pin labels where they are allowed
  and the volume has more than one slice).  On the aligned fast path the device takes the decision in k_trail_graph and
  the host takes it again from the per-slice sums: an encode that returns at all had the two agree (ckl_encoder_run
  fails otherwise), and the bytes say that both were right."""
  n = shape[0] * shape[1] * shape[2]
  h = n // 2
  pins, order = bool(kw.get("allow_pins")), int(kw.get("markov_model_order", 0))
  be = ckd.HipBackend(0)
  for k in (h - 1, h, h + 1):
    for place in ("head", "tail"):
      arr = tv.pairs_volume(shape, dtype, k, place)
      what = (k - h, place)
      want = checker.compress(arr, **kw)
      got = crackle_amd.compress(arr, **kw)
      head = crackle_amd.header(got)
      print(f"{_name(dtype, shape)} {_kw_name(kw)} k=H{k - h:+d} {place}: crack format {head.crack_format}, label format {head.label_format}, {len(got)} bytes, checker {len(want)}")
      assert head.crack_format == (tv.PERMISSIBLE if k < h else tv.IMPERMISSIBLE), what
      assert head.label_format == (tv.PINS if pins and k >= h and shape[2] > 1 else tv.FLAT), what
      assert head.markov_model_order == order and head.stored_data_width == 1
      assert got == want, what
      assert np.array_equal(crackle_amd.decompress(got), arr), what
      if dtype in (np.uint8, np.uint64):
        # device-resident volumes: the aligned one decides on the device, the view goes through k_stats
        for how, make in (("aligned", _aligned), ("unaligned", _unaligned)):
          t = make(arr)
          assert bytes(be.encode(t, shape, pins, True, order, None)) == want, (what, how)
          del t


# ---- c. where the maximum sits --------------------------------------------------------------------------------------
MAX_CASES = [(dt, value, width, shape) for dt, value, width in tv.MAX_VALUES for shape in tv.strip_shapes(dt)]


@pytest.mark.parametrize("dtype,value,width,shape", MAX_CASES, ids=[f"{_name(c[0], c[3])}-{c[1]}" for c in MAX_CASES])
def test_stored_width_wherever_the_maximum_sits(dtype, value, width, shape, checker):
  """One voxel decides the stored width: in the volume's first and last place, on either side of the full strip's last
  pixel column, in the full band's last row and in the band of one row, and at the start of the second slice."""
  for position in tv.POSITIONS:
    arr = tv.max_at(shape, dtype, value, position)
    got = crackle_amd.compress(arr)
    head = crackle_amd.header(got)
    print(f"{_name(dtype, shape)} {value} at {position}: stored width {head.stored_data_width}")
    assert head.stored_data_width == width, position
    assert got == checker.compress(arr), position


# ---- d. mode pooling re-encodes slice by slice ----------------------------------------------------------------------
POOL_CASES = [(dt, w) for dt in tv.DTYPES for w in tv.POOL_WIDTHS]


@pytest.mark.parametrize("dtype,width", POOL_CASES, ids=[f"{np.dtype(d).name}-{w}" for d, w in POOL_CASES])
def test_mode_pooling_decides_per_slice(dtype, width, checker):
  """ckl_mode_pooling_2x2x1 compresses every pooled slice from its own offset into one buffer (z * width * 5 * itemsize
  bytes: 200 bytes a slice for uint8 at width 40, so slice 1 is not 16-byte aligned).  The pooled slices are the three
  threshold slices, one on each side of H and one on it."""
  slices = tv.pooling_slices(width, dtype)
  binary = checker.compress(tv.pooling_input(width, dtype))
  got = operations._mode_pooling_slices(binary)
  assert got == checker.mode_pooling_2x2x1(binary)
  assert len(got) == 3
  for z, s in enumerate(slices):
    assert got[z] == checker.compress(np.asfortranarray(s.reshape(width, 5, 1))), z
  formats = [crackle_amd.header(b).crack_format for b in got]
  print(f"{np.dtype(dtype).name} width {width}: crack formats {formats}")
  assert formats == [tv.PERMISSIBLE, tv.IMPERMISSIBLE, tv.IMPERMISSIBLE]
